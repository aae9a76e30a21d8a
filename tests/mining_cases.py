"""Yardstick of the commonsense candidate mining: the reference's ``_get_related_top_k_predictions`` (``evaluator.py:375-416``)
restated literally on host arrays, plus the synthetic evaluator states of the property test.

``related_top_k_host`` is pinned to the real reference by ``tests/test_mining_cpu.py`` (fixture ``golden/mined_candidates.npz``, written
by ``golden/make_mining_golden.py`` from the reference's own method); the GPU tests then compare the device routes with it.
A *state* is a dict of numpy arrays in the evaluator's flat layout: candidates ``which, conf, pred, scat, ocat, sbox [n,4], obox [n,4]``
and targets ``which_t, rel_t, scat_t, ocat_t, sbox_t [t,4], obox_t [t,4]`` (``rel_t == -1``: not connected).
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
STATE_KEYS = ("which", "conf", "pred", "scat", "ocat", "sbox", "obox", "which_t", "rel_t", "scat_t", "ocat_t", "sbox_t", "obox_t")
TOP_KS = (1, 10, 63, 64, 65, 128)


def related_top_k_host(st, top_k, names=None, stats=None):
    """Per sorted unique image of ``st['which']`` the accepted (flat candidate position, rank j) pairs, in acceptance order.
    The loop is the reference's, statement by statement; the ranking is the project's defined one where the reference's unstable
    ``torch.argsort`` leaves the order open: equal confidences in append order, +0.0 ahead of -0.0 (``sgc_topk_per_image`` orders by
    bit pattern).  ``names=(object_names, relation_names)``: de-duplicate on the printed
    string as the reference does, else on the id triple.  ``stats['duplicates']`` (optional dict) counts the related candidates that
    were skipped because their triple was already in the image's list."""
    out = []
    for image in np.unique(st["which"]):
        cur = np.nonzero(st["which"] == image)[0]
        conf = st["conf"][cur].astype(np.float64)
        sorted_inds = np.lexsort((np.arange(len(cur)), np.signbit(conf) & (conf == 0), -conf))
        tcur = np.nonzero(st["which_t"] == image)[0]
        graph, seen = [], []
        for i in tcur:
            if st["rel_t"][i] == -1:
                continue
            if len(graph) >= 15:
                break
            for j in range(min(top_k, len(sorted_inds))):
                ind = cur[sorted_inds[j]]
                s_id, o_id = int(st["scat"][ind]), int(st["ocat"][ind])
                if (st["scat_t"][i] == s_id and np.sum(np.abs(st["sbox_t"][i] - st["sbox"][ind])) == 0) \
                        or (st["ocat_t"][i] == o_id and np.sum(np.abs(st["obox_t"][i] - st["obox"][ind])) == 0):
                    r_id = int(st["pred"][ind])
                    key = (s_id, r_id, o_id) if names is None else names[0][s_id] + " " + names[1][r_id] + " " + names[0][o_id]
                    if key not in seen:
                        graph.append((int(ind), j))
                        seen.append(key)
                    elif stats is not None:
                        stats["duplicates"] = stats.get("duplicates", 0) + 1
                if len(graph) >= 10:
                    break
        out.append(graph)
    return out


def lists_from_picks(st, picks, names):
    """(top_k_predictions, top_k_image_graphs) of ``get_related_top_k_predictions_parallel`` from the host loop's picks: strings and
    ``[subject_bbox, relation_id, object_bbox, confidence, j]`` edges (``evaluator.py:407-410``)."""
    preds, graphs = [], []
    for graph in picks:
        preds.append([names[0][int(st["scat"][p])] + " " + names[1][int(st["pred"][p])] + " " + names[0][int(st["ocat"][p])] for p, _ in graph])
        graphs.append([[st["sbox"][p].tolist(), int(st["pred"][p]), st["obox"][p].tolist(), float(st["conf"][p]), j] for p, j in graph])
    return preds, graphs


def crc_judge(predictions, context=None):
    """The fixture's deterministic judge: aligned when the CRC-32 of the string is even."""
    import zlib
    return [1 if zlib.crc32(s.encode()) % 2 == 0 else 0 for s in predictions]


def load_fixture():
    return dict(np.load(os.path.join(GOLDEN, "mined_candidates.npz"), allow_pickle=False))


def fixture_state(fx):
    return {k: fx["ref_" + k] for k in STATE_KEYS}


def fixture_lists(fx, top_k):
    """The reference's returned (predictions, graphs) and saved {path: edge list} of one ``top_k`` run, rebuilt from the arrays."""
    tag = "k%d_" % top_k
    cnt = fx[tag + "count"]
    preds, graphs = [], []
    for r, n in enumerate(cnt):
        preds.append([str(s) for s in fx[tag + "strings"][r, :n]])
        graphs.append([[fx[tag + "sbox"][r, e].tolist(), int(fx[tag + "rel"][r, e]), fx[tag + "obox"][r, e].tolist(),
                        float(fx[tag + "conf"][r, e]), int(fx[tag + "rank"][r, e])] for e in range(n)])
    saved = {}
    for i, path in enumerate(fx[tag + "saved_paths"]):
        row, sel = int(fx[tag + "saved_row"][i]), fx[tag + "saved_edges"][i]
        saved[str(path)] = [graphs[row][e] for e in sel[sel >= 0]]
    return preds, graphs, saved


def fixture_steps(fx):
    """The per-step arguments of ``Evaluator.accumulate`` that rebuild the reference's state (host tensors)."""
    import torch
    r0 = 0
    for b in fx["step_sizes"].tolist():
        sl = slice(r0, r0 + b)
        t = lambda k: torch.from_numpy(fx["step_" + k][sl])
        yield (t("which"), t("relation"), t("target"), None, t("conn"), t("scat"), t("ocat"), t("scat"), t("ocat"),
               t("sbox"), t("obox"), t("sbox"), t("obox"), t("iou"))
        r0 += b


def edges_equal(a, b):
    """Edge lists equal: boxes, relation id and rank as values, the confidence as the same f32."""
    if len(a) != len(b):
        return False
    for x, y in zip(a, b):
        if list(x[0]) != list(y[0]) or int(x[1]) != int(y[1]) or list(x[2]) != list(y[2]) or int(x[4]) != int(y[4]):
            return False
        if np.float32(x[3]) != np.float32(y[3]):
            return False
    return True


# ------------------------------------------------------------------------------------------------ synthetic states (property test)
# As in the reference's feed (train_utils.py:190-191) every candidate row carries the target of its own ordered pair: the target's
# classes and boxes are the row's, ``rel_t`` is its predicate or -1.  Targets are scanned in ROW order, candidates in RANK order.
def _finish(st):
    for k in ("scat", "ocat", "sbox", "obox", "which"):
        st[k + "_t"] = st[k].copy()
    for k in ("which", "pred", "scat", "ocat", "which_t", "rel_t", "scat_t", "ocat_t"):
        st[k] = np.asarray(st[k]).astype(np.int64)
    for k in ("sbox", "obox", "sbox_t", "obox_t"):
        st[k] = np.asarray(st[k]).astype(np.float32).reshape(-1, 4)
    st["conf"] = np.asarray(st["conf"]).astype(np.float32)
    return {k: st[k] for k in STATE_KEYS}


def _state(rng, n_per_image, connected=0.1, n_obj=6, n_cls=5, n_pred=7, image_ids=None, dup_objects=False):
    """Images of ``n_obj`` objects with classes < n_cls (few classes: equal classes on different boxes are common); rows = random
    ordered object pairs with a random predicate and confidence, a fraction ``connected`` of them with a target."""
    parts = {k: [] for k in ("which", "conf", "pred", "scat", "ocat", "sbox", "obox", "rel_t")}
    ids = list(range(len(n_per_image))) if image_ids is None else list(image_ids)
    for image, n in zip(ids, n_per_image):
        cats = rng.integers(0, n_cls, n_obj)
        boxes = rng.integers(0, 32, (n_obj, 4)).astype(np.float32)
        if dup_objects:                                   # two objects with the same class AND box: both match by value
            cats[1], boxes[1] = cats[0], boxes[0]
            cats[3], boxes[3] = cats[2], boxes[2]
        s, o = rng.integers(0, n_obj, n), rng.integers(0, n_obj, n)
        parts["which"].append(np.full(n, image)); parts["conf"].append(rng.standard_normal(n))
        parts["pred"].append(rng.integers(0, n_pred, n)); parts["scat"].append(cats[s]); parts["ocat"].append(cats[o])
        parts["sbox"].append(boxes[s]); parts["obox"].append(boxes[o])
        parts["rel_t"].append(np.where(rng.random(n) < connected, rng.integers(0, n_pred, n), -1))
    return _finish({k: np.concatenate(v) for k, v in parts.items()})


def _interleave(st, rng):
    """The images' rows interleaved as the reference's per-step appends leave them (order within an image kept)."""
    shuffled = rng.permutation(st["which"])               # which image owns every slot; its rows fill its slots in their own order
    new = np.empty(len(shuffled), dtype=np.int64)
    for image in np.unique(shuffled):
        new[np.nonzero(shuffled == image)[0]] = np.nonzero(st["which"] == image)[0]
    return {k: st[k][new] for k in STATE_KEYS}


def eleven_edge_state():
    """One image built so that rank 0 is first matched only AFTER the count reached 10.  The first target (row 0, pair 0->1) shares
    its subject with ranks 1..10 - ten predicates, ten accepts, the scan breaks at rank 10 - and not with rank 0 (pair 2->3).  The
    target of pair 2->4 comes next: examined against rank 0 alone under the `count >= 10` rule, it matches its subject: the 11th
    edge.  The targets after it (0->4: no match at rank 0; 2->3: rank 0 again, a duplicate) add nothing.  The rows that only carry
    those targets rank behind everything else and are never reached by the first target's scan."""
    boxes = np.asarray([[0, 4, 0, 4], [5, 9, 5, 9], [10, 14, 10, 14], [15, 19, 15, 19], [20, 24, 20, 24]], dtype=np.float32)
    cats = np.asarray([1, 2, 3, 4, 5])
    rows = [(0, 1, p, 4.0 - 0.1 * k, 3 if k == 0 else -1) for k, p in enumerate(list(range(10)) + [20, 21, 22, 23])]   # ranks 1..14
    rows += [(4, 3, 30, -9.0, -1), (2, 4, 31, -9.5, 7), (0, 4, 32, -10.0, 1), (2, 3, 40, 5.0, 2)]                          # last row: rank 0
    s, o = np.asarray([r[0] for r in rows]), np.asarray([r[1] for r in rows])
    return _finish(dict(which=np.zeros(len(rows)), conf=[r[3] for r in rows], pred=[r[2] for r in rows], scat=cats[s], ocat=cats[o],
                        sbox=boxes[s], obox=boxes[o], rel_t=[r[4] for r in rows]))


def property_states():
    """(name, state) pairs covering: images with fewer candidates than top_k / a single candidate / no connected target, all
    candidates -inf, many exact ties, duplicated (class, box) objects, image ids with gaps, up to 8 images and a few hundred
    candidates each, matches so dense that the `>= 10` cut binds, and the 11-edge case."""
    rng = np.random.default_rng(20240611)
    cases = []
    st = _state(rng, [300, 5, 70, 129, 64, 1, 200, 31], image_ids=[0, 2, 3, 6, 8, 9, 11, 12])
    cases.append(("ragged_8_images", _interleave(st, rng)))
    st = _state(rng, [40, 90, 150])
    st["conf"][:] = -np.inf
    cases.append(("all_minus_inf", _interleave(st, rng)))
    st = _state(rng, [200, 130, 66])
    st["conf"] = (np.round(st["conf"] * 1.5) / 1.5).astype(np.float32)          # a handful of distinct values: long runs of exact ties
    st["conf"][rng.random(len(st["conf"])) < 0.3] = -np.inf
    cases.append(("many_ties", _interleave(st, rng)))
    cases.append(("duplicate_objects", _interleave(_state(rng, [120, 80], dup_objects=True, n_cls=20, n_pred=30), rng)))
    st = _state(rng, [50, 60, 70], connected=0.2)
    st["rel_t"][st["which_t"] == 1] = -1                                         # image 1: no connected target
    cases.append(("no_connected_target", _interleave(st, rng)))
    st = _state(rng, [128, 127, 65], connected=0.5, n_obj=3, n_cls=2, n_pred=50)  # nearly every rank is related: the cut binds
    cases.append(("dense_matches", _interleave(st, rng)))
    st = _state(rng, [90, 40], connected=0.03, n_obj=12, n_cls=40, n_pred=50)     # sparse: few matches, long scans
    cases.append(("sparse_matches", _interleave(st, rng)))
    st = _state(rng, [300, 200, 129, 66], connected=0.01, n_obj=40, n_cls=150, n_pred=50)   # accepts at ranks past 64: both register sets
    cases.append(("high_ranks", _interleave(st, rng)))
    cases.append(("eleven_edges", eleven_edge_state()))
    return cases
