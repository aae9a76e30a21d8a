"""Host side of the SGDET / SGCLS metric tests: synthetic states for ``sgc_recall_accumulate_targets`` - ranked lists in
``sgc_scene_graph_topk``'s output layout over candidate objects, and a free-standing table of ground-truth triples with classes and
boxes of their own - and a numpy restatement of the counter loop of ``Evaluator.compute(predcls=False)`` (reference
``evaluator.py:272-277, 306-356``; labels through ``utils.compare_object_cat``, ``utils.py:355-373``, every IoU on the reference's
rasterised masks).  ``fixture_properties`` states what the fixtures reach, so that no case passes vacuously.  No GPU is needed here."""
import numpy as np

from oracle.relhead_oracle import compare_object_cat
from tests import metrics_cases as MC

F, R, C, IOU, TOP_K, KS = MC.F, MC.R, MC.C, MC.IOU, MC.TOP_K, MC.KS
POOL = (0, 50, 1, 5, 123, 14, 63, 60, 145, 108, 89, 7, 8)        # classes of the drawn state: mostly members of equivalence classes
PARTNER = {0: 50, 50: 0, 1: 5, 5: 1, 123: 14, 14: 123, 63: 123, 60: 145, 145: 60, 108: 89, 89: 108, 7: 8, 8: 60}     # 7, 8: no equivalent


def _grid_box(i):
    """Disjoint 4 x 4 boxes, seven to a row: two different objects of an image never reach IoU 0.5."""
    x0, y0 = 3 + 4 * (i % 7), 3 + 8 * (i // 7)
    return [x0, x0 + 4, y0, y0 + 4]


def _table(rows):
    """rows of (image, rel, scat, ocat, sbox, obox) -> the arrays of ``pairs.sg_target_table``."""
    col = lambda k, dt: np.asarray([r[k] for r in rows], dtype=dt)
    return dict(image=col(0, np.int32), rel=col(1, np.int64), scat=col(2, np.int64), ocat=col(3, np.int64),
                sbox=col(4, np.float32).reshape(-1, 4), obox=col(5, np.float32).reshape(-1, 4))


def crafted_state():
    """Four images with every special case at a chosen rank.  Image 0: 14 objects and 128 ranked candidates; image 1: 5 objects, 12
    candidates (-1 padding at every K); image 2: targets and no candidate; image 3: candidates and no target."""
    cls = [[0, 21, 14, 22, 7, 8, 9, 10, 30, 31, 32, 33, 34, 35], [60, 145, 61, 62, 200], [40, 41, 42], [43, 44, 45, 46]]
    off = np.concatenate([[0], np.cumsum([len(c) for c in cls])])
    cats = np.asarray([c for im in cls for c in im], dtype=np.int64)
    boxes = np.asarray([_grid_box(i) for im in cls for i in range(len(im))], dtype=np.float32)
    box = lambda b, i: boxes[off[b] + i].tolist()
    # image 0: fillers over the objects 8..13 (no target uses their classes), then the special candidates at their ranks
    pairs = [(s, o) for s in range(8, 14) for o in range(8, 14) if s != o]
    ranked0 = [(pairs[j % 30][0], pairs[j % 30][1], 40 + j // 30) for j in range(128)]
    special = {2: (5, 7, 9), 5: (0, 4, 3), 6: (4, 2, 8), 8: (1, 7, 55), 10: (1, 4, 14), 19: (1, 5, 4), 20: (3, 5, 5), 30: (5, 7, 10),
               49: (1, 6, 6), 50: (3, 6, 7), 70: (6, 7, 11), 110: (7, 6, 12)}
    for j, c in special.items():
        ranked0[j] = c
    ranked1 = [(2, 3, 22), (3, 2, 24), (1, 0, 25), (0, 1, 20), (2, 4, 26), (4, 2, 27), (3, 4, 28), (4, 2, 23), (0, 2, 29), (2, 0, 30),
               (1, 2, 31), (2, 1, 32)]
    ranked3 = [(0, 1, 1), (1, 2, 2), (2, 3, 3), (3, 0, 4)]
    ranked = [[(off[b] + s, off[b] + o, p) for s, o, p in lst] for b, lst in enumerate((ranked0, ranked1, [], ranked3))]
    frac = lambda bx: [v + 0.9 for v in bx]
    rows = [
        (0, 3, 50, 7, box(0, 0), box(0, 4)),             # hits rank 5 only through the symmetric group (0, 50); zero-shot by ITS classes
        (0, 8, 7, 123, box(0, 4), box(0, 2)),            # hits rank 6 only through the asymmetric key 123 -> 14
        (0, 10, 8, 10, box(0, 5), box(0, 7)),            # rank 2 has the labels and boxes with predicate 9; rank 30 has predicate 10
        (0, 55, 21, 10, box(0, 1), box(0, 7)),           # predicate >= R: in the totals, in no per-class counter
        (0, 14, 21, 7, frac(box(0, 1)), box(0, 4)),      # 7.9 -> 7: the target's box truncates onto the candidate's
        (0, 4, 21, 8, box(0, 1), box(0, 5)),             # hit at rank 19 = k - 1 for k = 20; zero-shot
        (0, 5, 22, 8, box(0, 3), box(0, 5)),             # hit at rank 20 = k
        (0, 6, 21, 9, box(0, 1), box(0, 6)),             # hit at rank 49
        (0, 7, 22, 9, box(0, 3), box(0, 6)),             # hit at rank 50
        (0, 11, 9, 10, box(0, 6), box(0, 7)),            # hit at rank 70: the second ballot trip
        (0, 12, 10, 9, box(0, 7), box(0, 6)),            # hit at rank 110: within no threshold
        (0, -1, 21, 8, box(0, 1), box(0, 5)),            # not connected
        (0, 13, 22, 10, box(0, 3), box(0, 7)),           # zero-shot, no candidate: a miss
        (0, 4, 21, 8, box(0, 2), box(0, 5)),             # the labels of rank 19 on another subject box: a miss
        (1, 20, 60, 145, box(1, 0), box(1, 1)),          # hit at rank 3
        (1, 21, 61, 62, box(1, 2), box(1, 3)),           # rank 0 has labels and boxes, no rank has the predicate
        (1, 23, 200, 61, box(1, 4), box(1, 2)),          # classes outside the equivalence table match by equality
        (1, 23, 201, 61, box(1, 4), box(1, 2)),          # ... and not otherwise
        (2, 1, 40, 41, box(2, 0), box(2, 1)),            # image without candidates: not counted as targets
        (2, 2, 41, 42, box(2, 1), box(2, 2)),
        (7, 1, 40, 41, box(2, 0), box(2, 1)),            # image out of range
        (-1, 1, 40, 41, box(2, 0), box(2, 1)),
    ]
    zs = {(50, 3, 7), (21, 4, 8), (22, 13, 10)}
    return dict(name="crafted", n_img=4, cats=cats, boxes=boxes, ranked=ranked, targets=_table(rows), zs=zs, F=F, R=R, C=C)


def drawn_state():
    """Three images (14, 6 and 9 objects) ranked from random confidences by ``metrics_cases.rank_host``; the second image's rows are
    all excluded, so it owns targets and no candidate.  The targets are the connected rows with their classes partly replaced by
    another class of the pool (an equivalent one where the class has one), their boxes partly given fractional parts or shifted by a
    cell, a few predicates set to -1 or moved past R."""
    g = np.random.default_rng(11)
    sizes = (14, 6, 9)
    objs = []
    for n in sizes:
        im = []
        for _ in range(n):
            x0, y0 = int(g.integers(0, F - 8)), int(g.integers(0, F - 8))
            im.append((POOL[int(g.integers(0, len(POOL)))], [x0, x0 + int(g.integers(2, 9)), y0, y0 + int(g.integers(2, 9))]))
        objs.append(im)
    st = MC.make_state("drawn", sizes, seed=12, connect=0.5, hit_frac=0.9, objects=objs)
    st["included"] = (st["image"] != 1).astype(np.uint8)
    rows = []
    for p in np.nonzero(st["directed"] != -1)[0]:
        s, o = int(st["sub_idx"][p]), int(st["obj_idx"][p])
        sc, oc, rel = int(st["cats"][s]), int(st["cats"][o]), int(st["directed"][p])
        if g.random() < 0.3:
            sc = PARTNER[sc]
        if g.random() < 0.3:
            oc = PARTNER[oc]
        sb, ob = st["boxes"][s].astype(np.float64), st["boxes"][o].astype(np.float64)
        u = g.random()
        if u < 0.4:
            sb, ob = sb + g.random(4) * 0.98, ob + g.random(4) * 0.98
        elif u < 0.6:
            sb = sb + np.asarray([1, 1, 0, 0])
        u = g.random()
        if u < 0.05:
            rel = -1
        elif u < 0.1:
            rel = R + int(g.integers(0, 5))
        rows.append((int(st["image"][p]), rel, sc, oc, sb.tolist(), ob.tolist()))
    tg = _table(rows)
    keep = np.nonzero((tg["rel"] >= 0) & (tg["rel"] < R))[0]           # a zero-shot set holds triples of real predicates only
    st["zs"] = {(int(tg["scat"][t]), int(tg["rel"][t]), int(tg["ocat"][t])) for t in keep[::2]}
    st["targets"] = tg
    return st


_STATES = None


def states():
    """(name, state) of the synthetic cases, built once.  A state holds ``cats`` / ``boxes`` of the candidate objects, ``targets`` (the
    table), ``zs`` and either explicit ranked lists (``ranked``) or the tables ``metrics_cases.rank_host`` ranks."""
    global _STATES
    if _STATES is None:
        _STATES = [(s["name"], s) for s in (crafted_state(), drawn_state())]
    return _STATES


def ranked_lists(st, K):
    """predicate / subject / object [n_img,K] int32 (-1 padded) and count [n_img], as ``sgc_scene_graph_topk`` writes them."""
    if "ranked" not in st:
        rk = MC.rank_host(st, K)
        return {k: rk[k] for k in ("predicate", "subject", "object", "count")}
    out = {k: np.full((st["n_img"], K), -1, dtype=np.int32) for k in ("predicate", "subject", "object")}
    out["count"] = np.zeros(st["n_img"], dtype=np.int32)
    for b, lst in enumerate(st["ranked"]):
        out["count"][b] = min(len(lst), K)
        for j, (s, o, p) in enumerate(lst[:K]):
            out["subject"][b, j], out["object"][b, j], out["predicate"][b, j] = s, o, p
    return out


def sg_counters(st, rk, use_equiv, top_k=TOP_K):
    """The counters after one ``Evaluator.compute(per_class=True, predcls=False)`` over the ranked lists and the target table, and per
    COUNTED target a dict of what the scan met.  The evaluator visits the images that own a candidate and, there, the targets with a
    predicate != -1; per-class counters exist for predicates below R only (the evaluator's tensors have R entries)."""
    tg = st["targets"]
    n_obj, T, n_k = int(st["boxes"].shape[0]), int(tg["rel"].shape[0]), len(top_k)
    shadow = dict(boxes=np.concatenate([st["boxes"], tg["sbox"], tg["obox"]]), F=st["F"])        # every box as an object of MC.iou
    z = lambda *s: np.zeros(s, dtype=np.int64)
    c = dict(hits=z(n_k), hits_pc=z(n_k, st["R"]), targets=z(1), targets_pc=z(st["R"]), zs_hits=z(n_k), zs_hits_pc=z(n_k, st["R"]),
             zs_targets=z(1), zs_targets_pc=z(st["R"]))
    same = (lambda p, t: compare_object_cat(p, t)) if use_equiv else (lambda p, t: int(p) == int(t))
    seen = []
    for b in range(st["n_img"]):
        cnt = int(rk["count"][b])
        if cnt == 0:
            continue
        for t in np.nonzero(tg["image"] == b)[0]:
            rel, sc, oc = int(tg["rel"][t]), int(tg["scat"][t]), int(tg["ocat"][t])
            if rel == -1:
                continue
            zs = (sc, rel, oc) in st["zs"]
            cls = 0 <= rel < st["R"]
            hit, wrong_ahead, labels = None, False, None
            for j in range(cnt):
                cs, co = int(rk["subject"][b, j]), int(rk["object"][b, j])
                if same(st["cats"][cs], sc) and same(st["cats"][co], oc):
                    if MC.iou(shadow, n_obj + t, cs) >= IOU and MC.iou(shadow, n_obj + T + t, co) >= IOU:
                        if rel == int(rk["predicate"][b, j]):
                            for i, k in enumerate(top_k):
                                if j < k:
                                    c["hits"][i] += 1
                                    c["zs_hits"][i] += zs
                                    if cls:
                                        c["hits_pc"][i, rel] += 1
                                        c["zs_hits_pc"][i, rel] += zs
                            hit, labels = j, (sc, int(st["cats"][cs]), oc, int(st["cats"][co]))
                            break
                        wrong_ahead = True
            c["targets"][0] += 1
            c["zs_targets"][0] += zs
            if cls:
                c["targets_pc"][rel] += 1
                c["zs_targets_pc"][rel] += zs
            seen.append(dict(t=int(t), image=b, hit=hit, wrong_ahead=wrong_ahead, labels=labels, zs=zs, rel=rel, cnt=cnt))
    return c, seen


def fixture_properties():
    """What the state set reaches, as a dict of booleans (all must hold; tests/test_sg_metrics_cpu.py asserts it)."""
    p = {k: False for k in ("equiv_symmetric", "equiv_asymmetric", "wrong_predicate_first", "second_ballot_trip", "rank_19", "rank_20",
                            "rank_49", "rank_50", "padded_image", "targets_without_candidates", "candidates_without_targets",
                            "not_connected_row", "predicate_past_R", "zero_shot_hit", "zero_shot_miss", "box_truncates")}
    for _, st in states():
        tg = st["targets"]
        p["not_connected_row"] |= bool((tg["rel"] == -1).any())
        for K in KS:
            rk = ranked_lists(st, K)
            _, on = sg_counters(st, rk, True)
            _, offl = sg_counters(st, rk, False)
            off_hit = {e["t"]: e["hit"] for e in offl}
            for b in range(st["n_img"]):
                n_t = int(((tg["image"] == b) & (tg["rel"] != -1)).sum())
                cnt = int(rk["count"][b])
                p["padded_image"] |= 0 < cnt < K and bool((rk["subject"][b, cnt:] == -1).all())
                p["targets_without_candidates"] |= cnt == 0 and n_t > 0
                p["candidates_without_targets"] |= cnt > 0 and n_t == 0
            for e in on:
                h = e["hit"]
                if h is not None:
                    sc, cs, oc, co = e["labels"]
                    only_equiv = off_hit[e["t"]] is None
                    p["equiv_symmetric"] |= only_equiv and ({sc, cs} == {0, 50} or {oc, co} == {0, 50})
                    p["equiv_asymmetric"] |= only_equiv and ({sc, cs} == {123, 14} or {oc, co} == {123, 14})
                    p["wrong_predicate_first"] |= e["wrong_ahead"]
                    p["second_ballot_trip"] |= h >= 64 and K >= 100 and e["cnt"] >= 100
                    for r in (19, 20, 49, 50):
                        p["rank_%d" % r] |= h == r
                    t = e["t"]
                    s_obj = int(rk["subject"][e["image"], h])
                    tb, cb = tg["sbox"][t], st["boxes"][s_obj]
                    p["box_truncates"] |= bool((tb != np.floor(tb)).any() and (np.floor(tb) == cb).all() and (np.round(tb) != cb).any())
                p["predicate_past_R"] |= e["rel"] >= st["R"]
                p["zero_shot_hit"] |= e["zs"] and h is not None and h < TOP_K[-1]
                p["zero_shot_miss"] |= e["zs"] and h is None
    return p
