"""Scoring API of the reference's kNN-based baselines on the HIP kernels.

  discrepancy_scores   lib/baselines/discrepancy_baseline.py:164-242   dis_x | dis_y | div_x | div_y
  clip_similarity      lib/baselines/run_clip_sim.py:235-248 (DistanceEvaluator.our_metric)
  cos_distance_topk / count_knn_distribution   lib/metrics/utils.py:198-233 (in-tree brute-force kNN)
  deep_knn_scores      lib/baselines/run_deepknn.py:255-261 (--dist_method deep_knn) on class or cluster labels
"""
import ctypes

import torch

from . import _lib
from .index import IndexFlatIP
from .ops import checked_labels, dev_f32, normalize_vectors, our_metric, ptr, stream_ptr


def discrepancy_scores(db, q_img, q_txt, k, method, is_train=False):
    """`db`: LemonDB built with dist_type='cosine' (the baseline only uses IndexFlatIP, :150-155).
    method: 'dis_x' | 'dis_y' | 'div_x' | 'div_y'.  Returns pred_score [nq] (float32, CUDA)."""
    if method not in ("dis_x", "dis_y", "div_x", "div_y"):
        raise NotImplementedError(method)
    assert db.metric == _lib.METRIC_IP, "discrepancy baselines are defined on the cosine (IP) indices"
    q_img, q_txt = dev_f32(q_img, "q_img"), dev_f32(q_txt, "q_txt")
    E = db.img if method.endswith("_x") else db.txt
    qv = q_img if method.endswith("_x") else q_txt
    out = torch.empty(q_txt.shape[0], dtype=torch.float32, device=db.device)
    lib = _lib.load()
    with torch.cuda.device(db.device):
        _lib.check(lib.lemon_discrepancy(0 if method.startswith("dis") else 1, db.index_txt._h, ptr(E), ptr(qv),
                                         ptr(q_txt), q_txt.shape[0], int(k), int(bool(is_train)), ptr(out),
                                         stream_ptr(db.device)), "lemon_discrepancy")
    return out


DISCREPANCY_METHODS = ("dis_x", "dis_y", "div_x", "div_y")       # the order of lemon_discrepancy_ks's method bits and output rows
MAX_SWEEP_K = 63                                                 # max + 1 <= LEMON_MAX_K (the cache and the train split search k + 1)


def _checked_ks(ks):
    try:
        ks = [int(k) for k in ks]
    except (TypeError, ValueError):
        raise ValueError(f"ks: {ks!r} is not a list of integers") from None
    if not ks:
        raise ValueError("ks: the list is empty")
    if any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"ks: {ks} is not strictly ascending")
    if ks[0] < 1 or ks[-1] > MAX_SWEEP_K:
        raise ValueError(f"ks: every knn_k must lie in 1 .. {MAX_SWEEP_K}, got {ks}")
    return ks


def discrepancy_cache(db, kmax):
    """The database's own text neighbours for the dis_* scores (discrepancy_baseline.py:165-169), once for every split and
    every knn_k <= kmax: int64 CUDA [n, kmax + 1].  It belongs to the rows `db` holds now; discrepancy_sweep refuses it after
    an add."""
    kmax = int(kmax)
    if not 1 <= kmax <= MAX_SWEEP_K:
        raise ValueError(f"kmax must lie in 1 .. {MAX_SWEEP_K}, got {kmax}")
    assert db.metric == _lib.METRIC_IP, "discrepancy baselines are defined on the cosine (IP) indices"
    cache = torch.empty((db.index_txt.ntotal, kmax + 1), dtype=torch.int64, device=db.device)
    with torch.cuda.device(db.device):
        _lib.check(_lib.load().lemon_discrepancy_cache(db.index_txt._h, kmax + 1, ptr(cache), stream_ptr(db.device)),
                   "lemon_discrepancy_cache")
    return cache


def discrepancy_sweep(db, q_img, q_txt, ks, methods=DISCREPANCY_METHODS, is_train=False, cache=None):
    """discrepancy_scores for every method of `methods` and every knn_k of `ks` (strictly ascending, 1 .. 63) from one text
    search and one pass over each query's neighbour pairs: float32 CUDA [len(methods), len(ks), nq], in the orders given, every
    element with the bits of discrepancy_scores(db, q_img, q_txt, k, method, is_train).
    cache: discrepancy_cache(db, kmax) with kmax >= max(ks), shared by the splits of a run; None builds it here when a dis_*
    method is asked for."""
    ks = _checked_ks(ks)
    methods = list(methods)
    if not methods:
        raise ValueError("methods: the list is empty")
    for m in methods:
        if m not in DISCREPANCY_METHODS:
            raise ValueError(f"methods: {m!r} is not one of {DISCREPANCY_METHODS}")
    assert db.metric == _lib.METRIC_IP, "discrepancy baselines are defined on the cosine (IP) indices"
    q_img, q_txt = dev_f32(q_img, "q_img"), dev_f32(q_txt, "q_txt")
    nq, n = q_txt.shape[0], db.index_txt.ntotal
    if db.img.shape[0] != n or db.txt.shape[0] != n or q_img.shape[0] != nq:
        raise ValueError(f"the text index holds {n} rows, the database embeddings {db.img.shape[0]} / {db.txt.shape[0]}; "
                         f"{q_img.shape[0]} image and {nq} text queries")
    bits = 0
    for m in methods:
        bits |= 1 << DISCREPANCY_METHODS.index(m)
    kc = 0
    if bits & 3:
        if cache is None:
            cache = discrepancy_cache(db, ks[-1])
        if not (torch.is_tensor(cache) and cache.is_cuda and cache.dtype == torch.int64 and cache.dim() == 2 and cache.is_contiguous()):
            raise ValueError("cache: expected the contiguous int64 CUDA tensor discrepancy_cache returns")
        if cache.shape[0] != n:
            raise ValueError(f"cache: built for {cache.shape[0]} database rows, the database holds {n}")
        if cache.shape[1] < ks[-1] + 1:
            raise ValueError(f"cache: {cache.shape[1]} columns, max(ks) + 1 = {ks[-1] + 1} are needed")
        kc = cache.shape[1]
    else:
        cache = None
    out = torch.empty((4, len(ks), nq), dtype=torch.float32, device=db.device)     # rows of methods not asked for stay unwritten
    ks_c = (ctypes.c_int32 * len(ks))(*ks)
    with torch.cuda.device(db.device):
        _lib.check(_lib.load().lemon_discrepancy_ks(db.index_txt._h, ptr(db.img), ptr(db.txt), ptr(q_img), ptr(q_txt), nq, ks_c,
                                                    len(ks), int(bool(is_train)), bits, ptr(cache), 0 if cache is None else cache.shape[0],
                                                    kc, ptr(out), stream_ptr(db.device)), "lemon_discrepancy_ks")
    return out[[DISCREPANCY_METHODS.index(m) for m in methods]]


def clip_similarity(first_modality_embeddings, second_modality_embeddings, dist="cosine"):
    """CLIP-similarity baseline score = paired distance of (un-normalised) image and text embeddings."""
    return our_metric(first_modality_embeddings, second_modality_embeddings, dist)


def clip_logits_confidence(img_embeds, class_text_embeds, noisy_label, dist="cosine"):
    """Zero-shot CLIP-logits baseline (lib/baselines/train_zero_shot_clip_baseline.py:207-224): for every image the
    softmax over ALL class prompts of 1 - our_metric(text_c, image), read at the image's noisy label -> confidence [n]
    (float32 CUDA; low confidence = likely mislabelled).  Embeddings are taken un-normalised, as the baseline does."""
    kind = {"cosine": 0, "euclidean": 1, "manhattan": 2}.get(dist)
    if kind is None:
        raise NotImplementedError(dist)
    q, c = dev_f32(img_embeds, "img_embeds"), dev_f32(class_text_embeds, "class_text_embeds")
    assert q.dim() == 2 and c.dim() == 2 and q.shape[1] == c.shape[1]
    lab = checked_labels(noisy_label, q.shape[0], c.shape[0], q.device)      # ValueError for a label outside [0, C)
    out = torch.empty(q.shape[0], dtype=torch.float32, device=q.device)
    lib = _lib.load()
    with torch.cuda.device(q.device):
        _lib.check(lib.lemon_class_confidence(kind, ptr(q), q.shape[0], q.shape[1], ptr(c), c.shape[0], ptr(lab), ptr(out),
                                              stream_ptr(q.device)), "lemon_class_confidence")
    return out


def cos_distance_topk(features, k):
    """values, indices of the k smallest cosine distances of every row to all rows (self included), as
    `cosDistance(features).topk(k, largest=False, sorted=True)` (lib/metrics/utils.py:198-212) without
    the N x N matrix: exact flat search on the normalised features."""
    f = normalize_vectors(dev_f32(features, "features"))
    index = IndexFlatIP(f.shape[1], f.device)
    index.add(f)
    D, I = index.search(f, k)
    return 1.0 - D, I


def count_knn_distribution(num_classes, min_similarity, feat_cord, label, k, norm="l2"):
    """lib/metrics/utils.py:205-233: per-sample class distribution of its k nearest neighbours, weighted
    by (1 - min_similarity - distance), with the self-distance patched to 2*v1 - v2 (:214)."""
    values, indices = cos_distance_topk(feat_cord, k)
    values = values.clone()
    values[:, 0] = 2.0 * values[:, 1] - values[:, 2]
    label = torch.as_tensor(label).to(values.device)
    knn_labels = label[indices]
    w = 1.0 - min_similarity - values
    cnt = torch.zeros((values.shape[0], num_classes), dtype=torch.float32, device=values.device)
    cnt.scatter_add_(1, knn_labels.long(), w)
    if norm == "l2":
        return torch.nn.functional.normalize(cnt, p=2.0, dim=1)
    if norm == "l1":
        return cnt / cnt.sum(1, keepdim=True)
    raise NameError("Undefined norm")


def label_disagreement(I, k, db_label, q_label, drop_self=False, in_db=None):
    """Fraction of the k kept neighbours of every query whose label differs from the query's (float32 [nq], CUDA).
    I: int64 [nq, kk] neighbour lists (kk >= k + drop_self); with drop_self the self-exclusion of run_lemon.py:257-263
    (drop result[0] where in_db, else result[-1]); I = -1 slots disagree, a query label of -1 matches nothing."""
    assert torch.is_tensor(I) and I.is_cuda and I.dim() == 2 and I.dtype == torch.int64
    I = I.contiguous()
    dev = I.device
    db = torch.as_tensor(db_label).to(device=dev, dtype=torch.int32).contiguous()
    ql = torch.as_tensor(q_label).to(device=dev, dtype=torch.int32).contiguous()
    assert ql.shape[0] == I.shape[0]
    mask = None
    if in_db is not None:
        mask = torch.as_tensor(in_db).to(device=dev, dtype=torch.uint8).contiguous()
        assert mask.shape[0] == I.shape[0]
    out = torch.empty(I.shape[0], dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().lemon_knn_label_disagreement(ptr(I), I.shape[0], I.shape[1], int(k), int(bool(drop_self)), ptr(mask),
                                                            ptr(db), db.shape[0], ptr(ql), ptr(out), stream_ptr(dev)),
                   "lemon_knn_label_disagreement")
    return out


def deep_knn_scores(index_img, q_img, q_label, db_label, k, is_train=False, in_db=None):
    """Deep-kNN baseline score (the --dist_method deep_knn of lib/baselines/run_deepknn.py:255-261): search the image index
    for k (+ 1 on the train split, whose queries are in the DB) neighbours and return the fraction whose (noisy) label
    differs from the query's.  Labels are class ids or the cluster ids of get_dataset(..., cluster_text=True)."""
    q = dev_f32(q_img, "q_img")
    _, I = index_img.search(q, int(k) + int(bool(is_train)))
    return label_disagreement(I, k, db_label, q_label, drop_self=is_train, in_db=in_db)
