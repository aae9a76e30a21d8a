"""Fused attention without a GPU: the float64 reference of the GPU tests against ``nn.MultiheadAttention``, the argument checks of
``attention.fused_mha``, the library export and the default-off wiring in ``detr.py``."""
import pytest
import torch
from torch import nn

from tests import attention_cases as AC


def _mha64(E, H, seed):
    torch.manual_seed(seed)
    mha = nn.MultiheadAttention(E, H).double().eval()
    with torch.no_grad():
        mha.in_proj_bias.normal_()
        mha.out_proj.bias.normal_()
    return mha


@pytest.mark.parametrize("masked", [False, True])
def test_reference_is_multihead_attention_in_float64(masked):
    """q = k = x + pos and value = x as detr.py calls the module: the reference between the projections is the module's attention."""
    E, H, L, B = 64, 2, 37, 3
    mha = _mha64(E, H, 1)
    x, pos = torch.randn(L, B, E, dtype=torch.float64), torch.randn(L, B, E, dtype=torch.float64)
    mask = None
    if masked:
        mask = torch.zeros(B, L, dtype=torch.bool)
        mask[0, 30:] = True
        mask[1, :5] = True
        mask[2, 3::2] = True
    with torch.no_grad():
        want = mha(x + pos, x + pos, value=x, key_padding_mask=mask)[0]
        w, b = mha.in_proj_weight, mha.in_proj_bias
        q = torch.nn.functional.linear(x + pos, w[:E], b[:E])
        k = torch.nn.functional.linear(x + pos, w[E:2 * E], b[E:2 * E])
        v = torch.nn.functional.linear(x, w[2 * E:], b[2 * E:])
        got = mha.out_proj(AC.reference(q, k, v, H, mask))
    assert float((got - want).abs().max()) <= 1e-12


def test_reference_gives_zeros_where_every_key_is_masked():
    q, k, v, mask = AC.make_inputs(AC.ALL_MASKED_CASE, torch.float32)
    ref = AC.reference(q, k, v, AC.ALL_MASKED_CASE.H, mask)
    assert torch.isfinite(ref).all() and float(ref[:, 1].abs().max()) == 0.0 and float(ref[:, 0].abs().max()) > 0
    q, k, v, mask = AC.make_inputs(AC.NO_KEYS_CASE, torch.float32)
    assert float(AC.reference(q, k, v, AC.NO_KEYS_CASE.H, mask).abs().max()) == 0.0


def test_random_cases_keep_an_unmasked_key_per_image():
    for c in AC.RANDOM_CASES + AC.HAZARD_CASES + [AC.FULL_CASE]:
        m = AC.make_mask(c)
        assert m is None or bool((~m).any(dim=1).all()), c.name
    first = AC.make_mask(AC.BY_NAME["first_tile_masked"])
    middle = AC.make_mask(AC.BY_NAME["middle_tile_masked"])
    assert bool(first[:, :AC.KEY_TILE].all()) and bool(middle[:, AC.KEY_TILE:2 * AC.KEY_TILE].all()) and not bool(middle[:, :AC.KEY_TILE].any())


def test_argument_errors_come_before_the_device_check():
    from scene_graph_commonsense_amd.attention import fused_mha
    q, k, v = torch.randn(5, 2, 64), torch.randn(7, 2, 64), torch.randn(7, 2, 64)
    ok_mask = torch.zeros(2, 7, dtype=torch.bool)
    bad = [
        dict(q=q.half(), k=k, v=v, num_heads=2),                                   # dtype mix
        dict(q=q.double(), k=k.double(), v=v.double(), num_heads=2),               # unsupported dtype
        dict(q=q, k=k, v=v, num_heads=4),                                          # E != 32 * num_heads
        dict(q=q, k=k, v=v, num_heads=0),
        dict(q=q, k=k[:, :1], v=v, num_heads=2),                                   # B mismatch
        dict(q=q, k=k, v=v[:6], num_heads=2),                                      # Lk mismatch
        dict(q=q[0], k=k, v=v, num_heads=2),                                       # not 3-D
        dict(q=q, k=k, v=v, num_heads=2, key_padding_mask=torch.zeros(2, 6, dtype=torch.bool)),       # mask shape
        dict(q=q, k=k, v=v, num_heads=2, key_padding_mask=torch.zeros(2, 7)),                         # mask dtype
        dict(q=q, k=k, v=v, num_heads=2, key_padding_mask=ok_mask, scale=float("inf")),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            fused_mha(**kw)
    if torch.cuda.is_available():
        with pytest.raises(ValueError):                                            # mask on another device than the tensors
            fused_mha(q, k, v, 2, key_padding_mask=ok_mask.cuda())
    with pytest.raises(RuntimeError):                                              # valid arguments, CPU tensors: no fallback
        fused_mha(q, k, v, 2, key_padding_mask=ok_mask)


def test_mha_forward_refuses_module_layouts_it_does_not_cover():
    from scene_graph_commonsense_amd.attention import mha_forward
    x = torch.randn(4, 2, 64)
    for mha in (nn.MultiheadAttention(64, 2, kdim=48, vdim=48), nn.MultiheadAttention(64, 2, batch_first=True),
                nn.MultiheadAttention(64, 2, add_bias_kv=True)):
        with pytest.raises(ValueError):
            mha_forward(mha, x, x, x)


def test_library_exports_sgc_mha_fwd():
    from scene_graph_commonsense_amd import _lib
    assert hasattr(_lib.load(), "sgc_mha_fwd")


def test_flag_moves_no_state_and_cpu_takes_the_unfused_line(monkeypatch):
    from scene_graph_commonsense_amd import attention
    from scene_graph_commonsense_amd.detr import DETR, build_detr101
    torch.manual_seed(0)
    plain = DETR(blocks=(1, 1, 1, 1), enc=1, dec=1).eval()
    fused = DETR(blocks=(1, 1, 1, 1), enc=1, dec=1).eval()
    fused.load_state_dict(plain.state_dict())
    assert fused.set_fused_attention(True) is fused
    layers = list(fused.transformer.encoder.layers) + list(fused.transformer.decoder.layers)
    assert all(l.fused_attention for l in layers)
    assert not any(l.fused_attention for l in list(plain.transformer.encoder.layers) + list(plain.transformer.decoder.layers))
    assert list(fused.state_dict().keys()) == list(plain.state_dict().keys())
    assert [n for n, _ in fused.named_modules()] == [n for n, _ in plain.named_modules()]

    def boom(*a, **kw):
        raise AssertionError("the kernel route was taken on the CPU")
    monkeypatch.setattr(attention, "fused_mha", boom)
    images = [torch.randn(3, 64, 96), torch.randn(3, 96, 64)]
    with torch.no_grad():
        a, b = plain(images), fused(images)
        assert torch.equal(a["pred_logits"], b["pred_logits"]) and torch.equal(a["pred_boxes"], b["pred_boxes"])
        sq = torch.randn(2, 3, 64, 64)
        assert torch.equal(plain.encode(sq), fused.encode(sq))
        assert torch.equal(plain.encode(sq), plain.encode(sq, fused_attention=True))
    assert not any(l.fused_attention for l in plain.transformer.encoder.layers)          # the per-call override is undone


def test_config_key_turns_the_flag_on():
    from scene_graph_commonsense_amd.detr import build_detr101
    from scene_graph_commonsense_amd.synthetic import HeadConfig
    args = HeadConfig().args()
    assert not build_detr101(args).transformer.encoder.layers[0].fused_attention
    args["models"]["feature_encoder_attention"] = "fused"
    model = build_detr101(args)
    assert all(l.fused_attention for l in list(model.transformer.encoder.layers) + list(model.transformer.decoder.layers))
