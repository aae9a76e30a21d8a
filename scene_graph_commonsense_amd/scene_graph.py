"""Scene-graph inference: "image + objects in, ranked top-K triples out" (reference ``evaluator.py:465-503``, the
``predicted_graph`` of ``save_visualization_results``).

``rank_scene_graphs`` is the device side: ONE kernel (``sgc_scene_graph_topk``, one workgroup per image) reads the head's
candidates, the connectivity, the overlap mask and the commonsense bitmaps in place, forms every candidate's confidence the
way the evaluator does (``evaluator.py:125-134,160-194,292``) and writes the stable descending top-K of every image.
``pair_loop.predict_scene_graphs`` runs it behind the fused forward; ``SceneGraphs.to_list`` is the host formatting.
The Recall@K ``Evaluator`` is not involved: no relation targets, no appended int64 copies, no host synchronisation.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional

import torch

from . import _lib

MAX_TOP_K = 128


@dataclass
class SceneGraphs:
    """Ranked triples of B images, K ranks each (device tensors unless built by hand; rows past ``count`` hold -1 / -inf)."""
    pair: torch.Tensor            # [B,K] int32  pair row of the minibatch (index into the forward's outputs)
    slot: torch.Tensor            # [B,K] int32  super-category slot of the candidate (0 for a flat head)
    predicate: torch.Tensor       # [B,K] int32
    subject: torch.Tensor         # [B,K] int32  flattened object index
    object: torch.Tensor          # [B,K] int32
    score: torch.Tensor           # [B,K] f32    (relation + category confidence) + log-sigmoid connectivity
    count: torch.Tensor           # [B] int32    min(K, candidates of the image)
    n_finite: torch.Tensor        # [B] int32    ranked entries with a finite score (the rest were filtered to -inf)
    subject_cat: Optional[torch.Tensor] = None     # [B,K] int64
    object_cat: Optional[torch.Tensor] = None
    subject_box: Optional[torch.Tensor] = None     # [B,K,4] raw grid boxes (x0,x1,y0,y1) as given
    object_box: Optional[torch.Tensor] = None
    image: Optional[torch.Tensor] = None           # [B] minibatch-local image index of every row
    feature_size: int = 32

    def to_list(self, heights, widths, names=None) -> List[List[dict]]:
        """Per image the reference's ``predicted_graph`` (``evaluator.py:482-503``): one dict per ranked edge with ``subject_id``,
        ``relation_id``, ``object_id``, ``bbox_sub``, ``bbox_obj`` and, with ``names=(object_names, relation_names)``, ``edge``.
        The reference's box scaling is kept as it is: box / feature_size, the FIRST TWO entries (x0, x1) times the image's height,
        the last two (y0, y1) times its width, ceil, int.  ``heights`` / ``widths`` are indexed by ``image``.  Pure host formatting."""
        if self.subject_cat is None or self.subject_box is None:
            raise ValueError("to_list needs subject_cat / object_cat / subject_box / object_box")
        host = lambda t: t.detach().cpu()
        count, pred = host(self.count).tolist(), host(self.predicate)
        scat, ocat, sbox, obox = host(self.subject_cat), host(self.object_cat), host(self.subject_box), host(self.object_box)
        image = list(range(len(count))) if self.image is None else host(self.image).tolist()
        out = []
        for b, n in enumerate(count):
            height, width = heights[image[b]], widths[image[b]]
            height, width = (height.item() if torch.is_tensor(height) else height), (width.item() if torch.is_tensor(width) else width)
            graph = []
            for r in range(int(n)):
                subject_id, relation_id, object_id = int(scat[b, r]), int(pred[b, r]), int(ocat[b, r])
                subject_bbox = sbox[b, r] / self.feature_size
                object_bbox = obox[b, r] / self.feature_size
                subject_bbox[:2] *= height
                subject_bbox[2:] *= width
                object_bbox[:2] *= height
                object_bbox[2:] *= width
                edge = {}
                if names is not None:
                    edge["edge"] = names[0][subject_id] + " " + names[1][relation_id] + " " + names[0][object_id]
                edge.update(subject_id=subject_id, relation_id=relation_id, object_id=object_id,
                            bbox_sub=subject_bbox.ceil().int().tolist(), bbox_obj=object_bbox.ceil().int().tolist())
                graph.append(edge)
            out.append(graph)
        return out


@dataclass
class MinedCandidates:
    """Commonsense candidates of B images (``pair_loop.mine_commonsense_candidates``): per image up to 11 ranked candidates that share
    an endpoint with a connected ground-truth triple, in acceptance order (reference ``evaluator.py:375-416``).  Device tensors; slots
    past ``count`` hold -1 / NaN."""
    pair: torch.Tensor            # [B,16] int32  pair row of the minibatch
    slot: torch.Tensor            # [B,16] int32  super-category slot of the candidate
    predicate: torch.Tensor       # [B,16] int32
    subject: torch.Tensor         # [B,16] int32  flattened object index
    object: torch.Tensor          # [B,16] int32
    rank: torch.Tensor            # [B,16] int32  the rank j of the candidate among the image's candidates
    score: torch.Tensor           # [B,16] f32    the candidate's confidence (no connectivity term)
    count: torch.Tensor           # [B] int32
    n_candidates: Optional[torch.Tensor] = None    # [B] int32  min(top_k, candidates of the image)
    cats: Optional[torch.Tensor] = None            # [n_obj] int64 object classes of the minibatch
    boxes: Optional[torch.Tensor] = None           # [n_obj,4] raw grid boxes (x0,x1,y0,y1) as given

    def to_lists(self, names, cats=None, boxes=None, all_images=False):
        """(top_k_predictions, top_k_image_graphs) as ``Evaluator.get_related_top_k_predictions_parallel`` returns them: per image the
        strings "subject predicate object" (``names`` = (object_names, relation_names)) and the edges [subject_bbox, relation_id,
        object_bbox, confidence, j].  Rows are the images that have at least one candidate, in order - the evaluator's sorted unique
        images - or, with ``all_images``, all B images.  ``cats`` / ``boxes``: per-object tables, default the minibatch's own.  The
        first host synchronisation of the route."""
        cats = self.cats if cats is None else cats
        boxes = self.boxes if boxes is None else boxes
        if cats is None or boxes is None:
            raise ValueError("to_lists needs the per-object cats and boxes")
        host = lambda t: torch.as_tensor(t).detach().cpu()
        cats, boxes = host(cats), host(boxes)
        count, pred, sub, obj = host(self.count).tolist(), host(self.predicate), host(self.subject), host(self.object)
        rank, score = host(self.rank).tolist(), host(self.score)
        has = [True] * len(count) if (all_images or self.n_candidates is None) else [n > 0 for n in host(self.n_candidates).tolist()]
        preds, graphs = [], []
        for b, n in enumerate(count):
            if not has[b]:
                continue
            p, g = [], []
            for e in range(n):
                s, o, r = int(sub[b, e]), int(obj[b, e]), int(pred[b, e])
                p.append(names[0][int(cats[s])] + " " + names[1][r] + " " + names[0][int(cats[o])])
                g.append([boxes[s].tolist(), r, boxes[o].tolist(), score[b, e].item(), rank[b][e]])
            preds.append(p)
            graphs.append(g)
        return preds, graphs


def _as(t, dtype, n, what):
    if t is None:
        return None
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError("rank_scene_graphs runs on the GPU (sgc_scene_graph_topk, no CPU fallback): %s must be a cuda tensor" % what)
    if t.numel() != n:
        raise ValueError("%s must hold %d entries, got %s" % (what, n, tuple(t.shape)))
    if t.dtype == torch.bool and dtype == torch.uint8:
        t = t.view(torch.uint8) if t.is_contiguous() else t.to(torch.uint8)
    return t.to(dtype).contiguous()


def rank_scene_graphs(cand_conf: torch.Tensor, cand_pred: torch.Tensor, conn: torch.Tensor, image_ptr: torch.Tensor, top_k: int = 20,
                      pair_list: Optional[torch.Tensor] = None, slot_major: bool = True, cat_conf: Optional[torch.Tensor] = None,
                      mask: Optional[torch.Tensor] = None, included: Optional[torch.Tensor] = None,
                      sub_idx: Optional[torch.Tensor] = None, obj_idx: Optional[torch.Tensor] = None,
                      cats: Optional[torch.Tensor] = None, bitmaps=None) -> SceneGraphs:
    """The ranked top-K candidates of every image from per-row candidates, e.g. ``BayesianHead.candidates`` (``cand_conf`` /
    ``cand_pred`` [M,3], or [M,1] / [M] for a flat head) and ``conn`` [M] = the LOG-SIGMOID connectivity of every row.
    ``image_ptr`` [B+1] int32: image b owns the rows ``image_ptr[b]:image_ptr[b+1]``, or, with ``pair_list``, the rows
    ``pair_list[image_ptr[b]:image_ptr[b+1]]`` (ascending).  Score = ``(cand_conf + cat_conf) + conn``; -inf where ``mask`` [M] is 0
    or ``bitmaps`` (``commonsense.TripletBitmaps``; needs ``sub_idx``, ``obj_idx`` [M] and ``cats`` [n_obj]) reject the triple; rows with
    ``included`` 0 are no candidates.  Ties rank in append order: ``slot_major=True`` is the order of ONE blocked append of all rows
    (``Evaluator.accumulate_candidates(..., call_sizes=[M])``: per image slot 0 of its rows, then slot 1, ...), ``False`` is
    (row, slot).  ``top_k`` <= 128.  No host synchronisation.  Returns ``SceneGraphs`` without categories and boxes."""
    if not (1 <= int(top_k) <= MAX_TOP_K):
        raise ValueError("top_k must be in 1..%d (one workgroup sorts an image's ranked window in LDS)" % MAX_TOP_K)
    if not torch.is_tensor(cand_conf) or not cand_conf.is_cuda:
        raise RuntimeError("rank_scene_graphs runs on the GPU (sgc_scene_graph_topk, no CPU fallback): cand_conf must be a cuda tensor")
    if cand_conf.dim() == 1:
        cand_conf = cand_conf[:, None]
    M, rep = int(cand_conf.shape[0]), int(cand_conf.shape[1])
    if rep not in (1, 3):
        raise ValueError("cand_conf must be [M,3] or [M,1], got %s" % (tuple(cand_conf.shape),))
    dev = cand_conf.device
    conf = _as(cand_conf, torch.float32, M * rep, "cand_conf")
    pred = _as(cand_pred, torch.int32, M * rep, "cand_pred")
    conn = _as(conn, torch.float32, M, "conn")
    B = int(image_ptr.numel()) - 1
    if B < 0:
        raise ValueError("image_ptr must hold B+1 entries")
    ptr = _as(image_ptr, torch.int32, B + 1, "image_ptr")
    lst = None if pair_list is None else _as(pair_list, torch.int32, int(pair_list.numel()), "pair_list")
    if bitmaps is not None and (sub_idx is None or obj_idx is None or cats is None):
        raise ValueError("the commonsense bitmaps need sub_idx, obj_idx and cats")
    cat_conf, mask, included = _as(cat_conf, torch.float32, M, "cat_conf"), _as(mask, torch.uint8, M, "mask"), _as(included, torch.uint8, M, "included")
    sub_idx, obj_idx = _as(sub_idx, torch.int32, M, "sub_idx"), _as(obj_idx, torch.int32, M, "obj_idx")
    cats = None if cats is None else _as(cats, torch.int64, int(cats.numel()), "cats")
    K = int(top_k)
    ints = torch.empty(5, max(B, 1), K, dtype=torch.int32, device=dev)
    score = torch.empty(max(B, 1), K, dtype=torch.float32, device=dev)
    cnt = torch.zeros(2, max(B, 1), dtype=torch.int32, device=dev)
    al = vi = None
    C = R = 0
    if bitmaps is not None:
        al, vi, C, R = bitmaps.aligned, bitmaps.violated, int(bitmaps.C), int(bitmaps.R)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().sgc_scene_graph_topk(
            _lib.ptr(conf), _lib.ptr(pred), rep, _lib.ptr(cat_conf), _lib.ptr(conn), _lib.ptr(mask), _lib.ptr(included), _lib.ptr(ptr),
            _lib.ptr(lst), _lib.ptr(sub_idx), _lib.ptr(obj_idx), _lib.ptr(cats), _lib.ptr(al), _lib.ptr(vi), C, R, B, K,
            1 if slot_major else 0, _lib.ptr(ints[0]), _lib.ptr(ints[1]), _lib.ptr(ints[2]), _lib.ptr(ints[3]), _lib.ptr(ints[4]),
            _lib.ptr(score), _lib.ptr(cnt[0]), _lib.ptr(cnt[1]), _lib.stream_ptr()), "sgc_scene_graph_topk")
    return SceneGraphs(pair=ints[0, :B], slot=ints[1, :B], predicate=ints[2, :B], subject=ints[3, :B], object=ints[4, :B],
                       score=score[:B], count=cnt[0, :B], n_finite=cnt[1, :B])


def attach_objects(graphs: SceneGraphs, cats: torch.Tensor, boxes: torch.Tensor, feature_size: int) -> SceneGraphs:
    """Fill ``subject_cat`` / ``object_cat`` / ``subject_box`` / ``object_box`` from per-object tables (``cats`` [n_obj] int64, ``boxes``
    [n_obj,4] raw grid boxes) through the ranked subject / object indices; padded ranks get -1."""
    ranked = graphs.subject >= 0
    pick = lambda table, idx: table[idx.clamp(min=0).long()]
    fill = lambda t, m: torch.where(m, t, torch.full_like(t, -1))
    if int(cats.numel()) == 0:
        B, K = graphs.subject.shape
        graphs.subject_cat = graphs.object_cat = torch.full((B, K), -1, dtype=torch.int64, device=graphs.subject.device)
        graphs.subject_box = graphs.object_box = torch.full((B, K, 4), -1, dtype=boxes.dtype, device=graphs.subject.device)
    else:
        graphs.subject_cat, graphs.object_cat = fill(pick(cats, graphs.subject), ranked), fill(pick(cats, graphs.object), ranked)
        graphs.subject_box = fill(pick(boxes, graphs.subject), ranked[..., None])
        graphs.object_box = fill(pick(boxes, graphs.object), ranked[..., None])
    graphs.feature_size = int(feature_size)
    return graphs
