"""Host side of the metric tests: a numpy restatement of the three counter updates that ``metrics.RecallMeter`` keeps on the device,
written from the reference's loops (``evaluator.py:280-367`` Recall@K / zero-shot, ``:697-773`` Top-3, ``:522-566`` OpenImages
precision) with the reference's own rasterised masks for every IoU, and synthetic ranked states in ``sgc_scene_graph_topk``'s
output layout that reach every branch of the kernels.  No GPU is needed here."""
import numpy as np

F, R, C = 32, 50, 150
SLOTS = ((0, 15), (15, 26), (26, 50))          # predicate ranges of the three super-categories
TOP_K = (20, 50, 100)
KS = (20, 100, 128)                            # ranking windows of the kernel test
IOU = 0.5


# ------------------------------------------------------------------------------------------------ synthetic scenes
def make_state(name, sizes, seed, cat_pool=C, box_pool=0, inf_frac=0.0, tie_levels=0, connect=0.5, hit_frac=0.8, drop=0.0,
               no_target_images=(), zero_area=0, clones=0, objects=None):
    """One minibatch as the kernels see it: per-object tables, per-pair-row tables in a shuffled order (the kernels may not depend
    on it; ``image`` says whose row it is), the head's candidates (``conf`` / ``cand_pred`` [P,3]; a masked pair is -inf in all
    slots) and directed targets (-1 = not connected).  ``objects``: explicit per-image lists of (class, box) instead of drawn ones."""
    g = np.random.default_rng(seed)
    pool = None
    if box_pool:
        x0, y0 = g.integers(0, F - 6, box_pool), g.integers(0, F - 6, box_pool)
        pool = np.stack([x0, x0 + g.integers(2, 7, box_pool), y0, y0 + g.integers(2, 7, box_pool)], 1)
    cats, boxes, image, sub, obj = [], [], [], [], []
    for b, n in enumerate(sizes):
        off = len(cats)
        for i in range(n):
            if objects is not None:
                c, box = objects[b][i]
            else:
                c = int(g.integers(0, cat_pool))
                if pool is not None:
                    box = pool[int(g.integers(0, box_pool))]
                else:
                    x0, y0 = int(g.integers(0, F - 4)), int(g.integers(0, F - 4))
                    box = [x0, x0 + int(g.integers(1, F - x0 + 1)), y0, y0 + int(g.integers(1, F - y0 + 1))]
                if i < zero_area:
                    box = [[7, 7, 2, 9], [9, 9, 1, 1], [5, 3, 4, 8]][i % 3]          # empty in x, in both, x1 < x0
                elif zero_area < i <= zero_area + clones:
                    c, box = cats[off + zero_area], boxes[off + zero_area]            # same class and box as the image's first drawn object
            cats.append(c)
            boxes.append([float(v) for v in box])
        for i in range(n):
            for j in range(n):
                if i != j:
                    image.append(b); sub.append(off + i); obj.append(off + j)
    P = len(image)
    perm = g.permutation(P)
    image, sub, obj = (np.asarray(a, dtype=np.int32)[perm] for a in (image, sub, obj))
    conf = g.normal(size=(P, 3)).astype(np.float32)
    if tie_levels:
        conf = (np.round(conf * tie_levels) / tie_levels).astype(np.float32)
    conf[g.random(P) < inf_frac] = -np.inf
    cand_pred = np.stack([g.integers(lo, hi, P) for lo, hi in SLOTS], 1).astype(np.int32)
    directed = np.full(P, -1, dtype=np.int32)
    connected = g.random(P) < connect
    own = cand_pred[np.arange(P), g.integers(0, 3, P)]
    directed[connected] = np.where(g.random(P) < hit_frac, own, g.integers(0, R, P))[connected]
    for b in no_target_images:
        directed[image == b] = -1
    included = (g.random(P) >= drop).astype(np.uint8) if drop else None
    cats = np.asarray(cats, dtype=np.int64)
    t = np.nonzero(directed != -1)[0]
    zs = {(int(cats[sub[p]]), int(directed[p]), int(cats[obj[p]])) for p in t[::2]}     # about half of the target triples
    return dict(name=name, n_img=len(sizes), cats=cats, boxes=np.asarray(boxes, dtype=np.float32).reshape(-1, 4), image=image, sub_idx=sub,
                obj_idx=obj, conf=conf, cand_pred=cand_pred, directed=directed, included=included, zs=zs, F=F, R=R, C=C)


def _row(st, b, s, o):
    return int(np.nonzero((st["image"] == b) & (st["sub_idx"] == s) & (st["obj_idx"] == o))[0][0])


def union_state():
    """Crafted OpenImages-style image: (a, b) against the target (a', b') has both box IoUs at 0.5 but the two targets lie on the same
    8 cells of the prediction's 24 (found, not found_union); (c, d) against the target (d, c) of two objects of one class has equal
    union masks and disjoint boxes (found_union, not found); (e, f) are empty boxes (union == 0 -> IoU 0, neither)."""
    objs = [[(1, [0, 4, 0, 4]), (2, [0, 4, 2, 6]), (1, [0, 4, 2, 4]), (2, [0, 4, 2, 4]), (3, [10, 14, 10, 14]), (3, [20, 24, 20, 24]),
             (4, [7, 7, 2, 9]), (4, [9, 9, 1, 1])],
            [(5, [1, 9, 1, 9]), (6, [3, 12, 2, 8]), (7, [0, 32, 0, 32])]]
    st = make_state("union_cases", (8, 3), seed=77, connect=0.0, objects=objs)
    st["conf"][:] = np.minimum(st["conf"], 0.0) - 1.0
    for k, (cs, co, ts, to, pred) in enumerate(((0, 1, 2, 3, 4), (4, 5, 5, 4, 17), (6, 7, 6, 7, 30), (0, 2, 0, 2, 8))):
        pc, pt = _row(st, 0, cs, co), _row(st, 0, ts, to)
        slot = [lo <= pred < hi for lo, hi in SLOTS].index(True)
        st["conf"][pc, slot], st["cand_pred"][pc, slot], st["directed"][pt] = 5.0 - k, pred, pred
    st["directed"][_row(st, 1, 8, 9)] = int(st["cand_pred"][_row(st, 1, 8, 9), 1])
    st["zs"] = {(1, 4, 2)}
    return st


_STATES = None


def states():
    """(name, state) of every synthetic case, built once."""
    global _STATES
    if _STATES is None:
        _STATES = [(s["name"], s) for s in (
            make_state("high_ranks", (14,), seed=1, connect=0.6, hit_frac=1.0),                       # 546 candidates: hits past rank 64
            make_state("ties_and_inf", (6, 5, 7), seed=2, cat_pool=3, box_pool=4, inf_frac=0.4, tie_levels=2, connect=0.7),
            make_state("ragged_8_images", (5, 2, 9, 3, 6, 0, 4, 8), seed=3, cat_pool=12, connect=0.5, drop=0.25, no_target_images=(2,)),
            make_state("top3_rule", (12, 5), seed=4, connect=0.6, hit_frac=1.0),                      # > 50 targets, < 20 targets
            make_state("zero_area_and_clones", (6, 4), seed=5, cat_pool=4, zero_area=2, clones=2, connect=0.8, hit_frac=1.0),
            union_state())]
    return _STATES


def image_lists(st):
    """(ptr [n_img+1], list [P]) int32: the pair rows of every image in ascending order."""
    lst = np.argsort(st["image"], kind="stable").astype(np.int32)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(st["image"], minlength=st["n_img"]))]).astype(np.int32)
    return ptr, lst


def rank_host(st, K, top3=False):
    """The ranked lists as ``sgc_scene_graph_topk`` writes them (stable descending, ties in (row, slot) order, rows that are not
    included are no candidates; -1 padded): pair, slot, predicate, subject, object [n_img,K] int32 and count [n_img].  ``top3``: one
    candidate per pair at the maximum of its three confidences."""
    ptr, lst = image_lists(st)
    out = {k: np.full((st["n_img"], K), -1, dtype=np.int32) for k in ("pair", "slot", "predicate", "subject", "object")}
    out["count"] = np.zeros(st["n_img"], dtype=np.int32)
    for b in range(st["n_img"]):
        rows = [int(p) for p in lst[ptr[b]:ptr[b + 1]] if st["included"] is None or st["included"][p]]
        cand = [(p, 0) for p in rows] if top3 else [(p, s) for p in rows for s in range(3)]
        score = np.asarray([st["conf"][p].max() if top3 else st["conf"][p, s] for p, s in cand], dtype=np.float32)
        order = np.argsort(-score, kind="stable")[:K]
        out["count"][b] = len(order)
        for j, c in enumerate(order):
            p, s = cand[int(c)]
            out["pair"][b, j], out["slot"][b, j], out["predicate"][b, j] = p, s, st["cand_pred"][p, s]
            out["subject"][b, j], out["object"][b, j] = st["sub_idx"][p], st["obj_idx"][p]
    return out


# ------------------------------------------------------------------------------------------------ the reference's loops
def _mask(st, o):
    cache = st.setdefault("_masks", {})
    if o not in cache:
        b = st["boxes"][o]
        m = np.zeros((st["F"], st["F"]), dtype=bool)
        m[int(b[2]):int(b[3]), int(b[0]):int(b[1])] = True                    # evaluator.py:85-88
        cache[o] = m
    return cache[o]


def _iou_masks(mt, mp):
    union = int((mt | mp).sum())
    return 0 if union == 0 else float(int((mt & mp).sum())) / float(union)     # evaluator.py:89-94


def iou(st, t, p):
    return _iou_masks(_mask(st, t), _mask(st, p))


def iou_union(st, p1, p2, t1, t2):
    return _iou_masks(_mask(st, t1) | _mask(st, t2), _mask(st, p1) | _mask(st, p2))     # evaluator.py:97-115


def _targets(st, b):
    """Connected targets of image b in the kept rows, and all its kept rows."""
    rows = [int(p) for p in np.nonzero(st["image"] == b)[0] if st["included"] is None or st["included"][p]]
    return [p for p in rows if st["directed"][p] != -1], rows


def recall_counters(st, rk, top_k=TOP_K, top3=False):
    """The counters after one ``compute()`` over the state (``evaluator.py:294-356``; Top-3 ``:704-766``) and, per target, what the
    scan met: (image, hit rank or None, saw a label-and-box match with another predicate before it, number of targets of its image)."""
    n_k = len(top_k)
    z = lambda *s: np.zeros(s, dtype=np.int64)
    c = dict(hits=z(n_k), hits_pc=z(n_k, st["R"]), targets=z(1), targets_pc=z(st["R"]), zs_hits=z(n_k), zs_hits_pc=z(n_k, st["R"]),
             zs_targets=z(1), zs_targets_pc=z(st["R"]))
    seen = []
    for b in range(st["n_img"]):
        tg, _ = _targets(st, b)
        num_target = len(tg)
        for p in tg:
            rel, ts, to = int(st["directed"][p]), int(st["sub_idx"][p]), int(st["obj_idx"][p])
            zs = (not top3) and (int(st["cats"][ts]), rel, int(st["cats"][to])) in st["zs"]
            hit, wrong_ahead = None, False
            for j in range(int(rk["count"][b])):
                cs, co = int(rk["subject"][b, j]), int(rk["object"][b, j])
                if st["cats"][ts] == st["cats"][cs] and st["cats"][to] == st["cats"][co]:
                    if iou(st, ts, cs) >= IOU and iou(st, to, co) >= IOU:
                        ok = rel in st["cand_pred"][rk["pair"][b, j]].tolist() if top3 else rel == int(rk["predicate"][b, j])
                        if ok:
                            for i, k in enumerate(top_k):
                                if j >= (max(k, num_target) if top3 else k):
                                    continue
                                c["hits"][i] += 1
                                c["hits_pc"][i, rel] += 1
                                if zs:
                                    c["zs_hits"][i] += 1
                                    c["zs_hits_pc"][i, rel] += 1
                            hit = j
                            break
                        wrong_ahead = True
            c["targets"][0] += 1
            c["targets_pc"][rel] += 1
            if zs:
                c["zs_targets"][0] += 1
                c["zs_targets_pc"][rel] += 1
            seen.append((b, hit, wrong_ahead and hit is not None, num_target, zs))
    return c, seen


def precision_counters(st, rk):
    """``compute_precision``'s counters (``evaluator.py:523-557``) over the first 20 ranks, and per ranked candidate (found, found_union)."""
    z = lambda: np.zeros(st["R"], dtype=np.int64)
    c = dict(ap=z(), ap_union=z(), num_ap=z())
    flags = []
    for b in range(st["n_img"]):
        tg, _ = _targets(st, b)
        for i in range(min(20, int(rk["count"][b]))):
            cs, co, pred = int(rk["subject"][b, i]), int(rk["object"][b, i]), int(rk["predicate"][b, i])
            found = found_union = False
            for p in tg:
                ts, to = int(st["sub_idx"][p]), int(st["obj_idx"][p])
                if st["cats"][cs] == st["cats"][ts] and st["cats"][co] == st["cats"][to]:
                    if pred == int(st["directed"][p]):
                        if iou(st, cs, ts) >= IOU and iou(st, co, to) >= IOU and not found:
                            c["ap"][pred] += 1
                            found = True
                        if iou_union(st, cs, co, ts, to) >= IOU and not found_union:
                            c["ap_union"][pred] += 1
                            found_union = True
                    if found and found_union:
                        break
            c["num_ap"][pred] += 1
            flags.append((found, found_union))
    return c, flags


def zero_shot_words(st):
    """The zero-shot set as the device bitmap (``commonsense.TripletBitmaps._pack``'s layout): uint32 words, bit (s*R + r)*C + o."""
    nbits = st["C"] * st["R"] * st["C"]
    bits = np.zeros((nbits + 31) // 32 * 32, dtype=np.uint64)
    for s, r, o in st["zs"]:
        bits[(s * st["R"] + r) * st["C"] + o] = 1
    return (bits.reshape(-1, 32) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
