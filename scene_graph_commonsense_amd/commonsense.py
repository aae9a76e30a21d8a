"""Commonsense triplet filter (reference ``evaluator.py:189-194,261-266``; ``train_utils.py:49-50``).

The reference tests ``tuple(triplet) in dict`` per candidate row on the host (a device->host copy and a Python
hash lookup per row).  Here the two triplet sets become device bitmaps over the num_classes x num_relations x
num_classes space (150*50*150 bits = 141 KB) and the filter is one HIP kernel over all candidates.

``TripletSets`` is the producer of those two sets: step 2 of ``run_mode prepare_cs`` (reference ``dataloader.py:168-244``), the
bookkeeping that turns the judged edges of the candidate mining (``Evaluator.get_related_top_k_predictions_parallel``) into the
commonsense-aligned and -violated triplet dictionaries.  Host code, once per image.
"""
from __future__ import annotations

import os

import numpy as np
import torch

from . import _lib


class TripletBitmaps:
    def __init__(self, aligned_keys, violated_keys, num_classes: int, num_relations: int, device):
        self.C, self.R = int(num_classes), int(num_relations)
        self.device = torch.device(device)
        self.aligned = self._pack(aligned_keys)
        self.violated = self._pack(violated_keys)

    def _pack(self, keys) -> torch.Tensor:
        # the layout that triplet_bits / triplet_bit read on the device (csrc/eval_geom.h): triplet (s, r, o) is bit (s*R + r)*C + o
        nbits = self.C * self.R * self.C
        nwords = (nbits + 31) // 32
        bits = np.zeros(nwords * 32, dtype=np.uint64)
        for (s, r, o) in keys:
            if 0 <= s < self.C and 0 <= o < self.C and 0 <= r < self.R:
                bits[(s * self.R + r) * self.C + o] = 1
        words = (bits.reshape(nwords, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)   # bit b of word w
        return torch.from_numpy(words.view(np.int32).copy()).to(self.device)

    @classmethod
    def from_masks(cls, aligned, violated, device) -> "TripletBitmaps":
        """The bitmaps of two dense bool arrays [C, R, C] (entry [s, r, o] = the triplet is in the set) - the same layout as
        ``_pack`` without a Python loop over the keys."""
        aligned, violated = (np.ascontiguousarray(np.asarray(m.cpu() if torch.is_tensor(m) else m, dtype=bool)) for m in (aligned, violated))
        if aligned.ndim != 3 or aligned.shape[0] != aligned.shape[2] or violated.shape != aligned.shape:
            raise ValueError("aligned and violated must be bool [C, R, C] of one shape")
        self = cls((), (), aligned.shape[0], aligned.shape[1], device)

        def pack(mask):
            bits = mask.reshape(-1)
            bits = np.concatenate((bits, np.zeros(-bits.size % 32, dtype=bool)))
            return torch.from_numpy(np.packbits(bits, bitorder="little").view("<u4").view(np.int32).copy()).to(self.device)
        self.aligned, self.violated = pack(aligned), pack(violated)
        return self

    def filter_(self, subject_cat: torch.Tensor, relation_pred: torch.Tensor, object_cat: torch.Tensor,
                confidence: torch.Tensor) -> torch.Tensor:
        """confidence[i] = -inf where the triplet is violated or not aligned (in place, GPU only)."""
        if not confidence.is_cuda:
            raise RuntimeError("the commonsense filter runs on the GPU (sgc_commonsense_filter); move the inputs to cuda")
        lib = _lib.load()
        s, r, o = (t.to(torch.int64).contiguous() for t in (subject_cat, relation_pred, object_cat))
        assert confidence.dtype == torch.float32 and confidence.is_contiguous()
        _lib.check(lib.sgc_commonsense_filter(_lib.ptr(s), _lib.ptr(r), _lib.ptr(o), _lib.ptr(confidence), int(confidence.numel()),
                                              _lib.ptr(self.aligned), _lib.ptr(self.violated), self.C, self.R,
                                              _lib.stream_ptr()), "sgc_commonsense_filter")
        return confidence


def _first_equal_box(box, bbox):
    """Index of the FIRST object whose box equals ``box`` in all entries, or None (reference ``utils.match_bbox``, 'pc' branch)."""
    box = torch.as_tensor(box)
    for idx, b in enumerate(bbox):
        if torch.sum(torch.abs(b - box)) == 0:
            return idx
    return None


class TripletSets:
    """The three dictionaries {(subject class, predicate, object class): count} of ``prepare_cs`` step 2 (``dataloader.py:53-57``)."""

    def __init__(self):
        self.triplets_train_gt = {}
        self.commonsense_aligned_triplets = {}
        self.commonsense_violated_triplets = {}
        self._finalized = False

    def add_image(self, categories, relationships, subj_or_obj, bbox, aligned_edges, violated_edges):
        """One image (``dataloader.py:168-218``): ``categories`` [n], ``relationships`` / ``subj_or_obj`` its triangular target lists
        (row i = object i+1 against objects 0..i; direction 1 = object i+1 is the subject, 0 = the object, anything else = no edge),
        ``bbox`` [n,4], and the two saved edge lists of the mining ([subject_bbox, relation_id, object_bbox, confidence, j]).  An edge
        counts under the classes of the FIRST objects whose boxes equal its two boxes exactly; it is skipped when both ends match the
        same index or either end matches none."""
        if self._finalized:
            raise RuntimeError("finalize() has merged the ground truth already")
        cat = lambda i: int(categories[i])
        for i, (rels, sos) in enumerate(zip(relationships, subj_or_obj)):
            for j, (rel, so) in enumerate(zip(rels, sos)):
                if so == 1:
                    key = (cat(i + 1), int(rel), cat(j))
                elif so == 0:
                    key = (cat(j), int(rel), cat(i + 1))
                else:
                    continue
                self.triplets_train_gt[key] = self.triplets_train_gt.get(key, 0) + 1
        for edges, table in ((aligned_edges, self.commonsense_aligned_triplets), (violated_edges, self.commonsense_violated_triplets)):
            for subject_bbox, relation_id, object_bbox, _, _ in edges:
                s, o = _first_equal_box(subject_bbox, bbox), _first_equal_box(object_bbox, bbox)
                if s == o or s is None or o is None:
                    continue
                key = (cat(s), relation_id, cat(o))
                table[key] = table.get(key, 0) + 1

    def finalize(self):
        """``save_all_triplets``' merge (``dataloader.py:226-233``), once: the ground-truth counts are added into the aligned set and
        every ground-truth key is removed from the violated set."""
        if not self._finalized:
            for k, v in self.triplets_train_gt.items():
                self.commonsense_aligned_triplets[k] = self.commonsense_aligned_triplets.get(k, 0) + v
            self.commonsense_violated_triplets = {k: v for k, v in self.commonsense_violated_triplets.items()
                                                  if k not in self.triplets_train_gt}
            self._finalized = True
        return self

    def save(self, directory, llm_model):
        """The two ``.pt`` dicts under the reference's names (``dataloader.py:239-244``); returns (aligned path, violated path)."""
        self.finalize()
        suffix = "_gpt4v" if llm_model == "gpt4v" else "_gpt3p5_temp"
        os.makedirs(directory, exist_ok=True)
        pa = os.path.join(directory, "commonsense_aligned_triplets%s.pt" % suffix)
        pv = os.path.join(directory, "commonsense_violated_triplets%s.pt" % suffix)
        torch.save(self.commonsense_violated_triplets, pv)
        torch.save(self.commonsense_aligned_triplets, pa)
        return pa, pv

    def bitmaps(self, device, num_classes: int = 150, num_relations: int = 50) -> "TripletBitmaps":
        """The device filter of ``train_cs`` / ``eval_cs`` straight from the sets, without the file round trip."""
        self.finalize()
        return TripletBitmaps(self.commonsense_aligned_triplets.keys(), self.commonsense_violated_triplets.keys(), num_classes,
                              num_relations, device)
