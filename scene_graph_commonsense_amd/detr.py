"""DETR-101 feature extractor and detector: what ``utils.build_detr101`` (``utils.py:88-120``) obtains from
``torch.hub.load('facebookresearch/detr:main', 'detr_resnet101')`` and what ``process_image_features`` (``train_utils.py:9-18``) and
``evaluate.py:309`` call on it - ``backbone(NestedTensor) -> (maps, pos)``, ``input_proj``, ``transformer.encoder(src,
src_key_padding_mask=, pos=)`` and the full ``forward(NestedTensor) -> {'pred_logits', 'pred_boxes'}`` - restated here so that
the drivers run without the hub download.

PARITY UNPINNED.  The hub code is a third-party dependency that is not vendored in the reference (and there is no network here), so
this module restates the published architecture of DETR (Carion et al. 2020: ResNet-101 with frozen batch-norm, sine position
embedding with normalisation, 6+6 post-norm transformer with learned queries, 3-layer box MLP).  What IS pinned against the
reference: the parameter / buffer names and their count (``datasets/vg_scene_graph_annot/detr101_key_after.txt``, kept as the data
fixture ``tests/golden/detr101_keys.txt``), i.e. the reference's checkpoints load with ``load_state_dict``; the layer wiring is
checked against ``torch.nn`` building blocks on the CPU (``tests/test_detr_cpu.py``).  This is plain PyTorch on ROCm (MIOpen /
hipBLASLt underneath) - the feature extractor is upstream of the hot path and frozen (``train_test.py:80-81``).  Opt-in
(``DETR.set_fused_attention``, default off): the 18 attention blocks through ``attention.mha_forward``, a flash-style HIP kernel
for their 8 heads of 32 channels, instead of ``nn.MultiheadAttention``'s materialised ``[B*8, L, L]`` scores."""
import math
import os
from typing import List, Optional

import torch
import torch.nn.functional as F
from torch import Tensor, nn

from . import attention


class NestedTensor:
    """Batch of images padded to a common size + padding mask (True = padding), as the reference's ``utils.NestedTensor``."""

    def __init__(self, tensors: Tensor, mask: Optional[Tensor]):
        self.tensors, self.mask = tensors, mask

    def to(self, device):
        return NestedTensor(self.tensors.to(device), None if self.mask is None else self.mask.to(device))

    def decompose(self):
        return self.tensors, self.mask


def nested_tensor_from_tensor_list(tensor_list: List[Tensor]) -> NestedTensor:
    """``utils.py:185-204``: zero-pad to the largest height / width of the batch, mask = True on the padding."""
    if tensor_list[0].ndim != 3:
        raise ValueError("not supported")
    c = tensor_list[0].shape[0]
    h = max(int(t.shape[1]) for t in tensor_list)
    w = max(int(t.shape[2]) for t in tensor_list)
    out = tensor_list[0].new_zeros(len(tensor_list), c, h, w)
    mask = torch.ones(len(tensor_list), h, w, dtype=torch.bool, device=out.device)
    for img, pad, m in zip(tensor_list, out, mask):
        pad[:, :img.shape[1], :img.shape[2]].copy_(img)
        m[:img.shape[1], :img.shape[2]] = False
    return NestedTensor(out, mask)


class FrozenBatchNorm2d(nn.Module):
    """Batch-norm with fixed statistics and affine parameters (buffers, no ``num_batches_tracked``)."""

    def __init__(self, n: int):
        super().__init__()
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))

    def forward(self, x: Tensor) -> Tensor:
        scale = self.weight * (self.running_var + 1e-5).rsqrt()
        shift = self.bias - self.running_mean * scale
        return x * scale.view(1, -1, 1, 1).to(x.dtype) + shift.view(1, -1, 1, 1).to(x.dtype)


class Bottleneck(nn.Module):
    """ResNet v1.5 bottleneck (stride on the 3x3), names as torchvision's."""

    def __init__(self, cin: int, width: int, stride: int, downsample: bool):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, width, 1, bias=False)
        self.bn1 = FrozenBatchNorm2d(width)
        self.conv2 = nn.Conv2d(width, width, 3, stride=stride, padding=1, bias=False)
        self.bn2 = FrozenBatchNorm2d(width)
        self.conv3 = nn.Conv2d(width, width * 4, 1, bias=False)
        self.bn3 = FrozenBatchNorm2d(width * 4)
        self.downsample = nn.Sequential(nn.Conv2d(cin, width * 4, 1, stride=stride, bias=False), FrozenBatchNorm2d(width * 4)) if downsample else None

    def forward(self, x: Tensor) -> Tensor:
        idt = x if self.downsample is None else self.downsample(x)
        out = F.relu(self.bn1(self.conv1(x)))
        out = F.relu(self.bn2(self.conv2(out)))
        return F.relu(self.bn3(self.conv3(out)) + idt)


class ResNetBody(nn.Module):
    """ResNet trunk up to layer4 (stride 32, 2048 channels); ``blocks`` = (3, 4, 23, 3) is ResNet-101."""

    def __init__(self, blocks=(3, 4, 23, 3)):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = FrozenBatchNorm2d(64)
        cin = 64
        for k, (n, width) in enumerate(zip(blocks, (64, 128, 256, 512))):
            layers = []
            for b in range(n):
                layers.append(Bottleneck(cin, width, stride=(2 if (b == 0 and k > 0) else 1), downsample=(b == 0)))
                cin = width * 4
            setattr(self, "layer%d" % (k + 1), nn.Sequential(*layers))
        self.num_channels = cin

    def forward(self, x: Tensor) -> Tensor:
        x = F.max_pool2d(F.relu(self.bn1(self.conv1(x))), 3, stride=2, padding=1)
        return self.layer4(self.layer3(self.layer2(self.layer1(x))))


class Backbone(nn.Module):
    def __init__(self, blocks=(3, 4, 23, 3)):
        super().__init__()
        self.body = ResNetBody(blocks)
        self.num_channels = self.body.num_channels
        for p in self.parameters():
            p.requires_grad_(False)                       # the reference never trains it (detr.eval(), no optimizer entry)

    def forward(self, t: NestedTensor) -> List[NestedTensor]:
        x = self.body(t.tensors)
        mask = F.interpolate(t.mask[None].float(), size=x.shape[-2:]).to(torch.bool)[0]
        return [NestedTensor(x, mask)]


class PositionEmbeddingSine(nn.Module):
    """Normalised 2-D sine embedding over the un-padded extent of each image (128 features per axis -> 256 channels)."""

    def __init__(self, num_pos_feats=128, temperature=10000.0, scale=2 * math.pi):
        super().__init__()
        self.num_pos_feats, self.temperature, self.scale = num_pos_feats, temperature, scale

    def forward(self, t: NestedTensor) -> Tensor:
        not_mask = ~t.mask
        y = not_mask.cumsum(1, dtype=torch.float32)
        x = not_mask.cumsum(2, dtype=torch.float32)
        eps = 1e-6
        y = y / (y[:, -1:, :] + eps) * self.scale
        x = x / (x[:, :, -1:] + eps) * self.scale
        k = torch.arange(self.num_pos_feats, dtype=torch.float32, device=t.tensors.device)
        dim_t = self.temperature ** (2 * torch.div(k, 2, rounding_mode="floor") / self.num_pos_feats)
        px, py = x[:, :, :, None] / dim_t, y[:, :, :, None] / dim_t
        px = torch.stack((px[..., 0::2].sin(), px[..., 1::2].cos()), dim=4).flatten(3)
        py = torch.stack((py[..., 0::2].sin(), py[..., 1::2].cos()), dim=4).flatten(3)
        return torch.cat((py, px), dim=3).permute(0, 3, 1, 2)


class Joiner(nn.Sequential):
    def __init__(self, backbone, position_embedding):
        super().__init__(backbone, position_embedding)
        self.num_channels = backbone.num_channels

    def forward(self, t: NestedTensor):
        maps = self[0](t)
        return maps, [self[1](m).to(m.tensors.dtype) for m in maps]


def _with_pos(x: Tensor, pos: Optional[Tensor]) -> Tensor:
    return x if pos is None else x + pos


class TransformerEncoderLayer(nn.Module):
    """Post-norm layer; the position embedding is added to queries and keys only.  ``fused_attention = True`` sends the attention
    through ``attention.mha_forward`` (the head-dim-32 HIP kernel) whenever ``attention.fused_route`` allows it."""
    fused_attention = False

    def __init__(self, d=256, nhead=8, ff=2048, dropout=0.1):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, nhead, dropout=dropout)
        self.linear1, self.linear2 = nn.Linear(d, ff), nn.Linear(ff, d)
        self.norm1, self.norm2 = nn.LayerNorm(d), nn.LayerNorm(d)
        self.dropout, self.dropout1, self.dropout2 = nn.Dropout(dropout), nn.Dropout(dropout), nn.Dropout(dropout)

    def forward(self, src, src_mask=None, src_key_padding_mask=None, pos=None):
        q = k = _with_pos(src, pos)
        if self.fused_attention and attention.fused_route(self.self_attn, src_mask, q, src):
            att = attention.mha_forward(self.self_attn, q, k, src, src_key_padding_mask)
        else:
            att = self.self_attn(q, k, value=src, attn_mask=src_mask, key_padding_mask=src_key_padding_mask)[0]
        src = self.norm1(src + self.dropout1(att))
        return self.norm2(src + self.dropout2(self.linear2(self.dropout(F.relu(self.linear1(src))))))


class TransformerEncoder(nn.Module):
    def __init__(self, n=6, **kw):
        super().__init__()
        self.layers = nn.ModuleList([TransformerEncoderLayer(**kw) for _ in range(n)])
        self.norm = None

    def forward(self, src, mask=None, src_key_padding_mask=None, pos=None):
        for layer in self.layers:
            src = layer(src, src_mask=mask, src_key_padding_mask=src_key_padding_mask, pos=pos)
        return src


class TransformerDecoderLayer(nn.Module):
    fused_attention = False                              # as TransformerEncoderLayer: self- and cross-attention through the HIP kernel

    def __init__(self, d=256, nhead=8, ff=2048, dropout=0.1):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, nhead, dropout=dropout)
        self.multihead_attn = nn.MultiheadAttention(d, nhead, dropout=dropout)
        self.linear1, self.linear2 = nn.Linear(d, ff), nn.Linear(ff, d)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(d), nn.LayerNorm(d), nn.LayerNorm(d)
        self.dropout, self.dropout1, self.dropout2, self.dropout3 = (nn.Dropout(dropout) for _ in range(4))

    def forward(self, tgt, memory, memory_key_padding_mask=None, pos=None, query_pos=None):
        q = k = _with_pos(tgt, query_pos)
        if self.fused_attention and attention.fused_route(self.self_attn, None, q, tgt):
            att = attention.mha_forward(self.self_attn, q, k, tgt)
        else:
            att = self.self_attn(q, k, value=tgt)[0]
        tgt = self.norm1(tgt + self.dropout1(att))
        cq, ck = _with_pos(tgt, query_pos), _with_pos(memory, pos)
        if self.fused_attention and attention.fused_route(self.multihead_attn, None, cq, ck, memory):
            att = attention.mha_forward(self.multihead_attn, cq, ck, memory, memory_key_padding_mask)
        else:
            att = self.multihead_attn(query=cq, key=ck, value=memory, key_padding_mask=memory_key_padding_mask)[0]
        tgt = self.norm2(tgt + self.dropout2(att))
        return self.norm3(tgt + self.dropout3(self.linear2(self.dropout(F.relu(self.linear1(tgt))))))


class TransformerDecoder(nn.Module):
    def __init__(self, n=6, d=256, **kw):
        super().__init__()
        self.layers = nn.ModuleList([TransformerDecoderLayer(d=d, **kw) for _ in range(n)])
        self.norm = nn.LayerNorm(d)

    def forward(self, tgt, memory, memory_key_padding_mask=None, pos=None, query_pos=None):
        inter = []
        for layer in self.layers:
            tgt = layer(tgt, memory, memory_key_padding_mask=memory_key_padding_mask, pos=pos, query_pos=query_pos)
            inter.append(self.norm(tgt))
        return torch.stack(inter)


class Transformer(nn.Module):
    def __init__(self, d=256, nhead=8, enc=6, dec=6, ff=2048, dropout=0.1):
        super().__init__()
        self.encoder = TransformerEncoder(enc, d=d, nhead=nhead, ff=ff, dropout=dropout)
        self.decoder = TransformerDecoder(dec, d=d, nhead=nhead, ff=ff, dropout=dropout)
        self.d_model, self.nhead = d, nhead
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def forward(self, src, mask, query_embed, pos_embed):
        b, c, h, w = src.shape
        src = src.flatten(2).permute(2, 0, 1)
        pos_embed = pos_embed.flatten(2).permute(2, 0, 1)
        query_embed = query_embed.unsqueeze(1).repeat(1, b, 1)
        mask = mask.flatten(1)
        memory = self.encoder(src, src_key_padding_mask=mask, pos=pos_embed)
        hs = self.decoder(torch.zeros_like(query_embed), memory, memory_key_padding_mask=mask, pos=pos_embed, query_pos=query_embed)
        return hs.transpose(1, 2), memory.permute(1, 2, 0).view(b, c, h, w)


class MLP(nn.Module):
    def __init__(self, cin, hidden, cout, n):
        super().__init__()
        dims = [cin] + [hidden] * (n - 1) + [cout]
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))

    def forward(self, x):
        for k, layer in enumerate(self.layers):
            x = layer(x) if k == len(self.layers) - 1 else F.relu(layer(x))
        return x


class DETR(nn.Module):
    """``detr_resnet101`` with ``class_embed`` sized by the caller (``utils.py:111-114``: 151 outputs for VG, 602 for OpenImages)."""

    def __init__(self, num_outputs=151, num_queries=100, blocks=(3, 4, 23, 3), d=256, nhead=8, enc=6, dec=6, ff=2048):
        super().__init__()
        self.backbone = Joiner(Backbone(blocks), PositionEmbeddingSine(d // 2))
        self.transformer = Transformer(d, nhead, enc, dec, ff)
        self.class_embed = nn.Linear(d, num_outputs)
        self.bbox_embed = MLP(d, d, 4, 3)
        self.query_embed = nn.Embedding(num_queries, d)
        self.input_proj = nn.Conv2d(self.backbone.num_channels, d, 1)

    def forward(self, samples):
        if isinstance(samples, (list, tuple)) or torch.is_tensor(samples):
            samples = nested_tensor_from_tensor_list(list(samples))
        maps, pos = self.backbone(samples)
        src, mask = maps[-1].decompose()
        hs = self.transformer(self.input_proj(src), mask, self.query_embed.weight, pos[-1])[0]
        return {"pred_logits": self.class_embed(hs)[-1], "pred_boxes": self.bbox_embed(hs).sigmoid()[-1]}

    def set_fused_attention(self, flag: bool = True) -> "DETR":
        """Route every attention block (6 encoder self-, 6 decoder self-, 6 decoder cross-attention) through the fused HIP kernel
        (``attention.mha_forward``) where ``attention.fused_route`` allows it.  A plain attribute: no parameter or buffer moves."""
        for layer in list(self.transformer.encoder.layers) + list(self.transformer.decoder.layers):
            layer.fused_attention = bool(flag)
        return self

    @torch.no_grad()
    def encode(self, images: Tensor, feature_size: Optional[int] = None, autocast: Optional[torch.dtype] = None,
               fused_attention: Optional[bool] = None) -> Tensor:
        """``process_image_features`` in one call: stacked images ``[B,3,H,W]`` -> encoder memory ``[B,256,H/32,W/32]``.
        ``autocast=torch.bfloat16`` runs the convolutions / GEMMs on the matrix cores in bf16 (the relation head reads the features
        as f16 anyway); the default keeps the reference's f32.  ``fused_attention`` overrides the layers' flag for this call.
        A list of images of unequal size is zero-padded and masked; a non-square map comes back as ``[B,256,h,w]``."""
        layers = list(self.transformer.encoder.layers)
        saved = [l.fused_attention for l in layers]
        try:
            if fused_attention is not None:
                for l in layers:
                    l.fused_attention = bool(fused_attention)
            return self._encode(images, feature_size, autocast)
        finally:
            for l, f in zip(layers, saved):
                l.fused_attention = f

    def _encode(self, images, feature_size, autocast):
        images = list(images)                                  # stacked, or a list of images of unequal size (zero-padded, masked)
        dev = images[0].device
        with torch.autocast(dev.type, dtype=autocast, enabled=autocast is not None):
            maps, pos = self.backbone(nested_tensor_from_tensor_list(images))
            src, mask = maps[-1].decompose()
            tok = self.input_proj(src).flatten(2).permute(2, 0, 1)
            mem = self.transformer.encoder(tok, src_key_padding_mask=mask.flatten(1), pos=pos[-1].flatten(2).permute(2, 0, 1))
        out = mem.permute(1, 2, 0).float()
        if feature_size is None and src.shape[-2] != src.shape[-1]:
            return out.reshape(-1, out.shape[1], src.shape[-2], src.shape[-1])
        fs = feature_size or int(round(math.sqrt(out.shape[-1])))
        return out.reshape(-1, out.shape[1], fs, fs)


def build_detr101(args) -> DETR:
    """``utils.build_detr101`` without the hub: the module above with 151 (VG) / 602 (OpenImages) class outputs; when the
    checkpoint named in ``args['models']`` exists it is loaded, renaming detectron2-style keys with the reference's two key lists
    (``detr101_key_before`` -> ``detr101_key_after``) exactly as ``utils.py:96-109`` does; otherwise the weights stay random
    (benchmarks, tests)."""
    vg = args["dataset"]["dataset"] == "vg"
    model = DETR(num_outputs=151 if vg else 602)
    path = args["models"].get("detr101_pretrained_vg" if vg else "detr101_pretrained_oiv6")
    if path and os.path.exists(path):
        state = torch.load(path, map_location="cpu")["model"]
        kb, ka = args["models"].get("detr101_key_before"), args["models"].get("detr101_key_after")
        if kb and ka and os.path.exists(kb) and os.path.exists(ka):
            before = [l.rstrip("\n") for l in open(kb)]
            after = [l.rstrip("\n") for l in open(ka)]
            present = [k for k in state if k in before]
            for idx, k in enumerate(present):
                state[after[idx]] = state.pop(k)
        model.load_state_dict(state, strict=False)           # every parameter except "criterion.empty_weight" (utils.py:115)
    if args["models"].get("feature_encoder_attention") == "fused":      # opt-in: the attention blocks on the HIP kernel (attention.py)
        model.set_fused_attention(True)
    return model
