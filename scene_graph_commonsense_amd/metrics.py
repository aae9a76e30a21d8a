"""Device-resident Recall@K / mR@K / zero-shot recall, Top-3 recall and OpenImages wmAP: ``RecallMeter``.

The state of the reference's ``Evaluator`` / ``Evaluator_Top3`` (``evaluator.py:15-586, 589-790``) between two ``compute()`` calls is
every candidate of the minibatch; what survives ``clear_data()`` is a handful of counters.  ``RecallMeter`` keeps only those
counters, as ONE contiguous int64 device tensor, and updates them behind the fused forward with kernels that read the forward's
outputs and the scene's tables in place:

* ``sgc_scene_graph_topk`` ranks every image's candidates (confidences, filters and tie order of ``evaluate_minibatch`` +
  ``Evaluator.compute()``: the call ``pair_loop.predict_scene_graphs`` makes);
* ``sgc_recall_accumulate`` (one wavefront per pair row) restates the hit test and the counter update of ``evaluator.py:306-356``
  and, for the Top-3 variant, ``:720-760``;
* ``sgc_precision_accumulate`` (one wavefront per image and rank < 20) restates ``evaluator.py:522-557``.

``update`` never synchronises with the host; ``compute`` / ``compute_top3`` / ``compute_precision`` read the counters once and apply
the evaluators' formulas, NaN handling included.  The counters run on across ``update`` calls as the evaluators' run on across
``clear_data()``; integer sums are order-independent, so two runs give identical bits.

SGDET / SGCLS (``evaluator.py:272-277, 306-356`` with ``predcls=False``): the targets are ground-truth triples with classes and boxes
of their own, the candidates live on the PREDICTED objects' pair rows, and labels match through the reference's equivalence classes
(``utils.py:355-373``).  ``update(sg_targets=..., cat_conf=...)`` takes them as one device table (``pairs.sg_target_table``) and counts
with ``sgc_recall_accumulate_targets`` (one wavefront per ground-truth triple); only the Recall@K and zero-shot counters move, as in
the reference's ``eval_sgd`` / ``eval_sgc``.  There is no CPU path: tensors must live on the GPU.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .evaluator import OIV6_PREDICATE_WEIGHT
from .scene_graph import MAX_TOP_K, rank_scene_graphs

MAX_TOP_KS = 8                  # thresholds per launch (METRIC_MAX_KS of csrc/kernels_metrics.hip)
PRECISION_RANKS = 20            # compute_precision ranks the top 20 of every image (evaluator.py:527)


def parse_triplet_keys(keys):
    """``zero_shot_triplets`` holds strings "s_r_o" (``evaluator.py:341``); tuples pass through."""
    out = []
    for k in keys:
        out.append(tuple(int(v) for v in k.split("_")) if isinstance(k, str) else tuple(int(v) for v in k))
    return out


def upload_sg_targets(table, dev):
    """``pairs.sg_target_table``'s numpy arrays as the device tensors ``RecallMeter.update(sg_targets=...)`` takes."""
    dtypes = (np.int32, np.int64, np.int64, np.int64, np.float32, np.float32)
    return tuple(torch.from_numpy(np.ascontiguousarray(a, dtype=d)).to(dev) for a, d in zip(table, dtypes))


def scene_boxes(scene, dev) -> torch.Tensor:
    """[n_obj,4] f32 device copy of the scene's raw boxes (x0,x1,y0,y1 as given: the evaluators' boxes), made once and kept on it."""
    if scene._bbox_raw_f32 is None:
        scene._bbox_raw_f32 = torch.from_numpy(np.ascontiguousarray(scene.bbox_raw, dtype=np.float32).reshape(-1, 4)).to(dev)
    return scene._bbox_raw_f32


class RecallMeter:
    """``RecallMeter(args, num_classes, iou_thresh=0.5, top_k=(20, 50, 100), device=...)`` - the arguments of ``Evaluator``
    (``num_classes`` = number of predicates) plus the device of the counters."""

    def __init__(self, args, num_classes: int, iou_thresh: float = 0.5, top_k: Sequence[int] = (20, 50, 100), device="cuda"):
        self.args = args
        self.top_k = [int(k) for k in top_k]
        if not self.top_k or len(self.top_k) > MAX_TOP_KS:
            raise ValueError("top_k must hold 1..%d thresholds" % MAX_TOP_KS)
        if not (1 <= self.top_k[-1] <= MAX_TOP_K):
            raise ValueError("top_k[-1] must be in 1..%d (one workgroup sorts an image's ranked window in LDS)" % MAX_TOP_K)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("RecallMeter keeps its counters on the GPU and updates them with HIP kernels (no CPU fallback)")
        self.num_classes = int(num_classes)
        self.iou_thresh = float(iou_thresh)
        self.hierar = bool(args["models"]["hierarchical_pred"])
        self.feature_size = int(args["models"]["feature_size"])
        self.num_object_classes = int(args["models"]["num_classes"])
        self.run_mode = args["training"]["run_mode"]
        self.dataset = args["dataset"]["dataset"]
        self._ks = (ctypes.c_int * len(self.top_k))(*self.top_k)
        n_k, R = len(self.top_k), self.num_classes
        # one tensor, named views: recall | zero-shot recall | top-3 recall (hits [n_k], hits_pc [n_k,R], targets [1], targets_pc [R]
        # each) | precision (ap, ap_union, num_ap [R] each)
        block = n_k + n_k * R + 1 + R
        self.counters = torch.zeros(3 * block + 3 * R, dtype=torch.int64, device=self.device)
        self._layout = {}
        o = 0
        for name in ("recall", "zero_shot", "top3"):
            for part, size, shape in (("hits", n_k, (n_k,)), ("hits_pc", n_k * R, (n_k, R)), ("targets", 1, (1,)), ("targets_pc", R, (R,))):
                self._layout[name + "." + part] = (o, size, shape)
                o += size
        for part in ("ap", "ap_union", "num_ap"):
            self._layout["precision." + part] = (o, R, (R,))
            o += R
        self._equiv = None                  # [160,160] u8 device copy of evaluator._equiv_matrix(), uploaded at the first SGDET / SGCLS update
        self.zero_shot = None               # [C*R*C bits] device bitmap of the zero-shot triplets (TripletBitmaps' layout)
        self._cs_keys, self._cs = None, None
        if self.dataset == "vg":
            from .commonsense import TripletBitmaps
            p = args["dataset"].get("zero_shot_triplets")
            zs = torch.load(p) if p and os.path.exists(p) else None          # as Evaluator.__init__: a missing file is an empty set
            bm = TripletBitmaps(parse_triplet_keys(zs if zs is not None else []), [], self.num_object_classes, R, self.device)
            self.zero_shot = bm.aligned
        if self.run_mode in ("train_cs", "eval_cs"):                         # the Evaluator's own commonsense filter (evaluator.py:76-81)
            suffix = "_gpt4v" if args["models"].get("llm_model") == "gpt4v" else ""
            d = args["dataset"]
            pa = d.get("commonsense_aligned_triplets", "triplets/commonsense_aligned_triplets%s.pt" % suffix)
            pv = d.get("commonsense_violated_triplets", "triplets/commonsense_violated_triplets%s.pt" % suffix)
            self._cs_keys = (list(torch.load(pa).keys()), list(torch.load(pv).keys()))

    # ------------------------------------------------------------------ state
    def view(self, name: str) -> torch.Tensor:
        """A named part of ``counters`` (``recall.hits``, ``zero_shot.targets_pc``, ``top3.hits_pc``, ``precision.ap``, ...)."""
        o, size, shape = self._layout[name]
        return self.counters[o:o + size].view(shape)

    def reset(self):
        self.counters.zero_()

    def _bitmaps(self, commonsense):
        if commonsense is not None or self._cs_keys is None:
            return commonsense
        if self._cs is None:
            from .commonsense import TripletBitmaps
            self._cs = TripletBitmaps(self._cs_keys[0], self._cs_keys[1], self.num_object_classes, self.num_classes, self.device)
        return self._cs

    # ------------------------------------------------------------------ update
    def update(self, scene, out, overlap: Optional[torch.Tensor] = None, included: Optional[torch.Tensor] = None, commonsense=None,
               top3: bool = True, directed: Optional[torch.Tensor] = None, *, sg_targets=None, cat_conf: Optional[torch.Tensor] = None):
        """Add one minibatch: ``scene`` (``pairs.DeviceScene`` with relation targets, or ``directed`` [P] given), ``out`` the forward's
        ``PairOutputs``, ``overlap`` [P] u8 the overlap mask (0 -> the pair's candidates rank at -inf), ``included`` [P] the pairs of the
        kept direction-steps (others are neither candidates nor targets), ``commonsense`` a ``commonsense.TripletBitmaps`` (default: the
        sets of ``args`` in run modes train_cs / eval_cs).  ``top3``: also the Top-3 counters, for a hierarchical head.  With
        ``dataset == 'oiv6'`` the precision counters are updated from the first 20 ranks of the same ranking - what ``compute()``
        followed by ``compute_precision()`` ranks.  No host synchronisation.
        ``cat_conf`` [P] f32: subject + object category confidence of every pair row, added to each of its candidates before the
        connectivity term (``Evaluator.accumulate_candidates(cat_confidence=...)``).
        ``sg_targets``: SGDET / SGCLS - the ground truth as a device table (image int32 [T], relation, subject class, object class
        int64 [T], subject box, object box f32 [T,4]: ``upload_sg_targets(pairs.sg_target_table(...))``) instead of ``directed``; the
        scene is then the PREDICTED objects' and labels match through the reference's equivalence classes.  Only ``recall.*`` and
        ``zero_shot.*`` move (``eval_sgd`` / ``eval_sgc`` record neither Top-3 nor wmAP)."""
        if not torch.is_tensor(out.cand_conf) or not out.cand_conf.is_cuda:
            raise RuntimeError("RecallMeter.update runs on the GPU (sgc_recall_accumulate, no CPU fallback): the forward's outputs must "
                               "be cuda tensors")
        dev = out.cand_conf.device
        if cat_conf is not None:
            if not torch.is_tensor(cat_conf) or not cat_conf.is_cuda:
                raise RuntimeError("RecallMeter.update runs on the GPU (no CPU fallback): cat_conf must be a cuda tensor")
            if int(cat_conf.numel()) != int(scene.n_pairs):
                raise ValueError("cat_conf must hold one value per pair row")
            cat_conf = cat_conf.to(torch.float32).contiguous()
        if sg_targets is not None:
            if directed is not None:
                raise ValueError("sg_targets and directed are two ways to give the ground truth: pass one of them")
            return self._update_sg(scene, out, overlap, included, commonsense, sg_targets, cat_conf, dev)
        directed = scene.directed if directed is None else directed
        if directed is None:
            raise ValueError("the metrics need relation targets: flatten the scene from a batch with relationships / subj_or_obj")
        if not directed.is_cuda:
            raise RuntimeError("RecallMeter.update runs on the GPU (no CPU fallback): directed must be a cuda tensor")
        P = int(scene.n_pairs)
        if P == 0:
            return
        directed = directed.to(torch.int32).contiguous()
        g, ptr, lst, boxes, included, logsig = self._rank(scene, out, overlap, included, commonsense, cat_conf, dev)
        B, K, R, n_k = int(ptr.numel()) - 1, self.top_k[-1], self.num_classes, len(self.top_k)
        lib = _lib.load()
        n_obj = int(scene.cats.numel())
        thr = ctypes.c_double(self.iou_thresh)

        def accumulate(g, name, cand_pred, n_pred, img_targets, zs):
            v = lambda part: _lib.ptr(self.view(name + "." + part))
            z = (lambda part: _lib.ptr(self.view("zero_shot." + part))) if zs is not None else (lambda part: _lib.ptr(None))
            _lib.check(lib.sgc_recall_accumulate(
                _lib.ptr(g.pair), _lib.ptr(g.predicate), _lib.ptr(g.subject), _lib.ptr(g.object), _lib.ptr(g.count), B, K,
                _lib.ptr(cand_pred), n_pred, _lib.ptr(scene.cats), _lib.ptr(boxes), n_obj, _lib.ptr(scene.sub_idx), _lib.ptr(scene.obj_idx),
                _lib.ptr(scene.image), _lib.ptr(directed), _lib.ptr(included), P, _lib.ptr(img_targets), self._ks, n_k, _lib.ptr(zs),
                self.num_object_classes, R, self.feature_size, thr, v("hits"), v("hits_pc"), v("targets"), v("targets_pc"), z("hits"),
                z("hits_pc"), z("targets"), z("targets_pc"), _lib.stream_ptr()), "sgc_recall_accumulate")

        with torch.cuda.device(dev):
            accumulate(g, "recall", None, 1, None, self.zero_shot)
            if self.dataset == "oiv6":
                _lib.check(lib.sgc_precision_accumulate(
                    _lib.ptr(g.predicate), _lib.ptr(g.subject), _lib.ptr(g.object), _lib.ptr(g.count), B, K, min(PRECISION_RANKS, K),
                    _lib.ptr(ptr), _lib.ptr(lst), _lib.ptr(scene.cats), _lib.ptr(boxes), n_obj, _lib.ptr(scene.sub_idx),
                    _lib.ptr(scene.obj_idx), _lib.ptr(directed), _lib.ptr(included), P, R, self.feature_size, thr,
                    _lib.ptr(self.view("precision.ap")), _lib.ptr(self.view("precision.ap_union")),
                    _lib.ptr(self.view("precision.num_ap")), _lib.stream_ptr()), "sgc_precision_accumulate")
            if top3 and self.hierar:
                # Evaluator_Top3: one candidate per pair at the maximum of its three confidences, no commonsense filter
                # (evaluator.py:697-718); a hit for rank < max(k, connected targets of the image)
                cand_pred = out.cand_pred.to(torch.int32).contiguous()
                g3 = rank_scene_graphs(out.cand_conf.max(dim=1)[0], cand_pred[:, 0], logsig, ptr, top_k=K, pair_list=lst, slot_major=False,
                                       mask=overlap, included=included, sub_idx=scene.sub_idx, obj_idx=scene.obj_idx, cats=scene.cats)
                is_target = directed != -1
                if included is not None:
                    is_target &= included.bool()
                img_targets = torch.zeros(B, dtype=torch.int32, device=dev).index_add_(0, scene.image.long(), is_target.int())
                accumulate(g3, "top3", cand_pred, 3, img_targets, None)

    def _rank(self, scene, out, overlap, included, commonsense, cat_conf, dev):
        """What every update starts with: the ranked lists of the minibatch's candidates (``sgc_scene_graph_topk``) and the tables they
        were ranked from - (lists, image ptr, image pair list, raw boxes, included as u8, log-sigmoid connectivity)."""
        from .pair_loop import image_pair_lists
        ptr, lst = image_pair_lists(scene)
        boxes = scene_boxes(scene, dev)
        if included is not None:
            included = (included.view(torch.uint8) if included.dtype == torch.bool else included.to(torch.uint8)).contiguous()
        # torch's own log(sigmoid(x)), as the evaluator feed forms it: the ranked scores are bit for bit the evaluator's confidences
        logsig = torch.log(torch.sigmoid(out.connectivity))
        g = rank_scene_graphs(out.cand_conf, out.cand_pred, logsig, ptr, top_k=self.top_k[-1], pair_list=lst, slot_major=False,
                              cat_conf=cat_conf, mask=overlap, included=included, sub_idx=scene.sub_idx, obj_idx=scene.obj_idx,
                              cats=scene.cats, bitmaps=self._bitmaps(commonsense))
        return g, ptr, lst, boxes, included, logsig

    def _update_sg(self, scene, out, overlap, included, commonsense, sg_targets, cat_conf, dev):
        from .evaluator import _equiv_matrix
        if len(sg_targets) != 6:
            raise ValueError("sg_targets is (image, relation, subject class, object class, subject box, object box)")
        for t in sg_targets:
            if not torch.is_tensor(t) or not t.is_cuda:
                raise RuntimeError("RecallMeter.update runs on the GPU (sgc_recall_accumulate_targets, no CPU fallback): the target "
                                   "table must be cuda tensors")
        T = int(sg_targets[0].numel())
        if any(int(t.numel()) != n * T for t, n in zip(sg_targets, (1, 1, 1, 1, 4, 4))):
            raise ValueError("the arrays of sg_targets disagree in length: [T] image, relation and classes, [T,4] boxes")
        P = int(scene.n_pairs)
        if P == 0 or T == 0:
            return
        t_image = sg_targets[0].to(torch.int32).contiguous()
        t_rel, t_scat, t_ocat = (t.to(torch.int64).contiguous() for t in sg_targets[1:4])
        t_sbox, t_obox = (t.to(torch.float32).contiguous() for t in sg_targets[4:6])
        if self._equiv is None:
            self._equiv = torch.from_numpy(_equiv_matrix().astype(np.uint8)).to(self.device)
        # (cand_conf + cat_conf) + log(sigmoid(connectivity)): bit for bit the evaluator's confidences with predcls=False
        g, ptr, _, boxes, _, _ = self._rank(scene, out, overlap, included, commonsense, cat_conf, dev)
        B, K, R, n_k = int(ptr.numel()) - 1, self.top_k[-1], self.num_classes, len(self.top_k)
        v = lambda part: _lib.ptr(self.view("recall." + part))
        z = (lambda part: _lib.ptr(self.view("zero_shot." + part))) if self.zero_shot is not None else (lambda part: _lib.ptr(None))
        with torch.cuda.device(dev):
            _lib.check(_lib.load().sgc_recall_accumulate_targets(
                _lib.ptr(g.predicate), _lib.ptr(g.subject), _lib.ptr(g.object), _lib.ptr(g.count), B, K, _lib.ptr(scene.cats),
                _lib.ptr(boxes), int(scene.cats.numel()), _lib.ptr(t_image), _lib.ptr(t_rel), _lib.ptr(t_scat), _lib.ptr(t_ocat),
                _lib.ptr(t_sbox), _lib.ptr(t_obox), T, _lib.ptr(self._equiv), int(self._equiv.shape[0]), self._ks, n_k,
                _lib.ptr(self.zero_shot), self.num_object_classes, R, self.feature_size, ctypes.c_double(self.iou_thresh), v("hits"),
                v("hits_pc"), v("targets"), v("targets_pc"), z("hits"), z("hits_pc"), z("targets"), z("targets_pc"), _lib.stream_ptr()),
                "sgc_recall_accumulate_targets")

    # ------------------------------------------------------------------ host reads
    def _host(self):
        h = self.counters.cpu()
        return lambda name: h[self._layout[name][0]:self._layout[name][0] + self._layout[name][1]].view(self._layout[name][2])

    def _recall(self, part, name, per_class):
        # evaluator.py:358-367: result_dict[k] / max(num_connected_target, 1e-3); per class f32 hits / targets (0 / 0 = NaN), nanmean
        hits, targets = part(name + ".hits").tolist(), float(part(name + ".targets")[0])
        hits_pc, targets_pc = part(name + ".hits_pc").float(), part(name + ".targets_pc").float()
        if not per_class:                   # the evaluators count per class only when asked to
            hits_pc = torch.zeros_like(hits_pc)
        recall_k = [float(h) / max(targets, 1e-3) for h in hits]
        recall_k_per_class = [hits_pc[i] / targets_pc for i in range(len(self.top_k))]
        return recall_k, recall_k_per_class, [torch.nanmean(r) for r in recall_k_per_class]

    def compute(self, per_class: bool = False):
        """The 6-tuple of ``Evaluator.compute``: (recall, recall per class, mean recall, and the three zero-shot twins - None unless
        ``dataset == 'vg'``).  ``per_class=False`` reports the per-class hits as zeros, as an evaluator never asked for them does."""
        part = self._host()
        res = self._recall(part, "recall", per_class)
        zs = self._recall(part, "zero_shot", per_class) if self.dataset == "vg" else (None, None, None)
        return res + zs

    def compute_top3(self, per_class: bool = False):
        """The 3-tuple of ``Evaluator_Top3.compute``."""
        return self._recall(self._host(), "top3", per_class)

    def compute_precision(self):
        """(wmAP_rel, wmAP_phr) of ``Evaluator.compute_precision`` (``evaluator.py:559-566``)."""
        part = self._host()
        weight = torch.tensor(OIV6_PREDICATE_WEIGHT) + 1
        num = part("precision.num_ap").float()
        ppc = part("precision.ap").float() / num
        not_nan = torch.logical_not(torch.isnan(ppc))
        wmp = torch.nansum(ppc * weight) / torch.sum(weight[not_nan])
        ppcu = part("precision.ap_union").float() / num
        wmpu = torch.nansum(ppcu * weight) / torch.sum(weight[not_nan])
        return wmp, wmpu
