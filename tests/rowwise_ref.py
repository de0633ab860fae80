"""float64 restatement of the row-wise scoring kernels (lemon_amd/csrc/rowwise.hip) and the two token-assembly kernels
(lemon_amd/csrc/encoder.hip): test helper, numpy / torch only, nothing from the library.  tests/test_rowwise_host.py checks
these functions against sklearn, scipy, torch.nn.functional and the recorded fixtures on a machine without a GPU;
tests/test_gpu_rowwise.py holds the kernels to them.

Also here: the FLOAT32 reference "the way the reference project computes it" (sklearn's pairwise functions on float32
arrays, the diagonal of the full matrix, scipy.special.softmax), whose own error against float64 sets the bar for the
kernels that have no bit-exact contract."""
import math

import numpy as np

U = 2.0 ** -24                      # unit roundoff of float32
FLOOR_REL = 2.4e-7                  # 2 ulp of float32, relative: the bar where the float32 reference lands exactly
MARGIN = 4.0                        # a kernel may be this much worse than the float32 reference (another summation order)
MODES = {1: "1 - dot", 2: "sum (a-b)^2", 3: "euclidean", 4: "manhattan", 5: "cosine"}
KIND_OF_MODE = {5: 0, 3: 1, 4: 2}   # lemon_paired_metric's kind for k_rowchain<MODE>
KIND_NAMES = ("cosine", "euclidean", "manhattan")


def f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- K1 -------------------------------------------------------------------------------------------------------------------
def normalize_rows(x):
    """x / max(|x|, 1e-12) per row (F.normalize(p=2, dim=1, eps=1e-12))"""
    x = f64(x)
    nrm = np.sqrt((x * x).sum(1, keepdims=True))
    return x / np.maximum(nrm, 1e-12)


def ulps(got32, ref64):
    """|got - fp32(ref)| in units of the spacing of fp32(ref) (subnormals included); non-finite `got` counts as inf"""
    r32 = f64(ref64).astype(np.float32)
    with np.errstate(invalid="ignore"):
        e = np.abs(f64(got32) - f64(r32)) / f64(np.spacing(np.abs(r32)))
    return np.where(np.isfinite(f64(got32)), e, np.inf)


# ---- K2 -------------------------------------------------------------------------------------------------------------------
def cosine_distance(dot, na, nb):
    """1 - dot / (sqrt(na) sqrt(nb)); a row of norm zero has similarity 0 (sklearn's normalize() leaves it as it is)"""
    den = np.sqrt(na) * np.sqrt(nb)
    with np.errstate(invalid="ignore", divide="ignore"):
        return 1.0 - np.where(den == 0.0, 0.0, dot / np.where(den == 0.0, 1.0, den))


def paired(mode, a, b):
    """row i of a against row i of b: float64 value [n] and the chain's error bracket sum_k |term_k| [n] (for mode 5 the
    bracket is already carried through the quotient: see paired_chain_bound)"""
    a, b = f64(a), f64(b)
    if mode == 1:
        return 1.0 - (a * b).sum(1)
    if mode == 2:
        return ((a - b) ** 2).sum(1)
    if mode == 3:
        return np.sqrt(((a - b) ** 2).sum(1))
    if mode == 4:
        return np.abs(a - b).sum(1)
    if mode == 5:
        return cosine_distance((a * b).sum(1), (a * a).sum(1), (b * b).sum(1))
    raise ValueError(mode)


def paired_chain_bound(mode, a, b):
    """|error| of a float32 evaluation that sums d terms in ANY order: d 2^-24 sum_k |term_k| for every sum, carried through
    the tail (sqrt, quotient), + 2 ulp of the result for the tail operations and the rounding of the terms themselves"""
    a, b = f64(a), f64(b)
    d = a.shape[1]
    val = paired(mode, a, b)
    tail = 2.0 * f64(np.spacing(np.abs(val).astype(np.float32)))
    if mode in (1, 5):
        s_dot = d * U * np.abs(a * b).sum(1)
        if mode == 1:
            return s_dot + tail
        na, nb = (a * a).sum(1), (b * b).sum(1)
        den = np.sqrt(na) * np.sqrt(nb)
        ok = den > 0
        den = np.where(ok, den, 1.0)
        cos = np.where(ok, (a * b).sum(1) / den, 0.0)
        # d(dot / sqrt(na nb)) = ddot / den - cos (dna / 2 na + dnb / 2 nb), with dna <= d U na (all terms positive)
        return np.where(ok, s_dot / den + np.abs(cos) * d * U, 0.0) + np.maximum(tail, 2.0 * 2.0 ** -23)
    if mode in (2, 3):
        s = ((a - b) ** 2).sum(1)
        e = d * U * s
        if mode == 2:
            return e + tail
        return np.where(s > 0, e / (2.0 * np.sqrt(np.where(s > 0, s, 1.0))), 0.0) + tail
    if mode == 4:
        return d * U * np.abs(a - b).sum(1) + tail
    raise ValueError(mode)


def sk_paired_metric(kind, a, b):
    """DistanceEvaluator.our_metric (lib/metrics/distance_metrics.py:48-73) on float32 arrays: the diagonal of sklearn's full
    pairwise matrix, in whatever dtype sklearn returns"""
    from sklearn.metrics.pairwise import cosine_similarity, euclidean_distances, manhattan_distances
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if kind == 0:
        return 1 - np.diagonal(cosine_similarity(a, b))
    if kind == 1:
        return np.diagonal(euclidean_distances(a, b))
    if kind == 2:
        return np.diagonal(manhattan_distances(a, b))
    raise ValueError(kind)


def reference_bar(ref32_err, scale):
    """what a kernel's error may be, element-wise: MARGIN x the float32 reference's own worst error against float64, and
    never less than 2 ulp of the value (`scale`: |value| for absolute errors, 1 for relative ones)"""
    return np.maximum(MARGIN * float(ref32_err), FLOOR_REL * f64(scale))


# ---- K2' and the zero-shot confidence ---------------------------------------------------------------------------------------
def class_distances(kind, img, cls):
    """[n, C] float64 distance of every image row to every class row; kind 0 cosine, 1 euclidean, 2 manhattan (our_metric),
    'ip' 1 - dot, 'l2' squared euclidean (run_lemon.py:244-248 on normalised embeddings)"""
    v, t = f64(img), f64(cls)
    if kind == "ip":
        return 1.0 - v @ t.T
    if kind == 0:
        return cosine_distance(v @ t.T, (v * v).sum(1)[:, None], (t * t).sum(1)[None, :])
    diff = v[:, None, :] - t[None, :, :]
    if kind == "l2":
        return (diff ** 2).sum(2)
    if kind == 1:
        return np.sqrt((diff ** 2).sum(2))
    if kind == 2:
        return np.abs(diff).sum(2)
    raise ValueError(kind)


def softmax_rows(z):
    z = f64(z)
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def _take(p, labels):
    """p[i, labels[i]] the way numpy indexes: IndexError for a label >= C, a negative label counts from the end"""
    return p[np.arange(p.shape[0]), np.asarray(labels, dtype=np.int64)]


def d1_normalized(metric, q_img, cls_txt, noisy_label):
    """softmax_c(dist(img_i, cls_c))[label_i], run_lemon.py:244-248; metric 'ip' (--dist_type cosine) or 'l2'"""
    return _take(softmax_rows(class_distances(metric, q_img, cls_txt)), noisy_label)


def d1_chain_bound(metric, q_img, cls_txt):
    """relative error bound [n] of k_d1_normalized's float32 evaluation: the distances are float32 chains (error Ez, see
    paired_chain_bound), z - max is rounded once, expf is good to 2 ulp, the sum of the C exponentials takes at most
    16 + 6 additions per lane, one division.  A softmax entry moves by at most 2 max|dz| relative."""
    v, t = f64(q_img), f64(cls_txt)
    n, C, d = v.shape[0], t.shape[0], v.shape[1]
    z = class_distances(metric, v, t)
    if metric == "ip":
        ez = d * U * (np.abs(v) @ np.abs(t).T) + 4.0 * U * np.maximum(np.abs(z), 1.0)
    else:
        ez = d * U * z + 4.0 * U * z
    spread = (z.max(1, keepdims=True) - z)
    return 2.0 * (ez + U * spread).max(1) + (2 * 2 + 22 + 1) * 2.0 * U


def class_confidence(kind, img, cls_txt, noisy_label):
    """softmax_c(1 - our_metric(cls_c, img_i))[label_i], lib/baselines/train_zero_shot_clip_baseline.py:207-224"""
    return _take(softmax_rows(1.0 - class_distances(kind, img, cls_txt)), noisy_label)


def sk_class_confidence(kind, img, cls_txt, noisy_label):
    """the same the way the reference runs it, on float32 arrays: per image, our_metric(text embeddings, the image repeated
    C times) -> scipy.special.softmax(1 - dist) -> the entry of the noisy label"""
    from scipy.special import softmax
    img, cls_txt = np.ascontiguousarray(img, np.float32), np.ascontiguousarray(cls_txt, np.float32)
    out = []
    for i in range(img.shape[0]):
        rep = np.repeat(img[i][None, :], cls_txt.shape[0], 0)
        out.append(softmax(1 - sk_paired_metric(kind, cls_txt, rep))[noisy_label[i]])
    return np.array(out)


# ---- K5 -------------------------------------------------------------------------------------------------------------------
HP_ORDER = ("beta", "gamma", "tau_1_n", "tau_2_n", "tau_1_m", "tau_2_m")


def score(rec, hp):
    """lib/metrics/utils.py:47-82 in float64: (score, d_n, d_m); rec holds float32 arrays d_1 [n] and D_n, dists_tr_n, dists_n,
    D_m, dists_tr_m, dists_m [n, k]; hp a dict or the six values in HP_ORDER.  inf x 0 gives NaN, as in the reference."""
    if isinstance(hp, dict):
        hp = [hp[h] for h in HP_ORDER]
    beta, gamma, t1n, t2n, t1m, t2m = (float(h) for h in hp)
    k = rec["D_n"].shape[1]
    with np.errstate(over="ignore", invalid="ignore"):
        wn = np.exp(-t1n * f64(rec["D_n"])) * np.exp(-t2n * f64(rec["dists_tr_n"])) * f64(rec["dists_n"])
        wm = np.exp(-t1m * f64(rec["D_m"])) * np.exp(-t2m * f64(rec["dists_tr_m"])) * f64(rec["dists_m"])
        dn = np.array([math.fsum(r) if np.isfinite(r).all() else r.sum() for r in wn]) / k
        dm = np.array([math.fsum(r) if np.isfinite(r).all() else r.sum() for r in wm]) / k
        return f64(rec["d_1"]) + beta * dn + gamma * dm, dn, dm


# ---- token assembly ---------------------------------------------------------------------------------------------------------
def vision_tokens(patches, cls, pos):
    """float64 [batch, n_tokens, width] = cat(cls, patches) + pos (torch tensors in, float64 out)"""
    import torch
    p = patches.double()
    x = torch.cat([cls.double().reshape(1, 1, -1).expand(p.shape[0], 1, p.shape[2]), p], 1)
    return x + pos.double()[None, :, :]


def vision_tokens_ln(patches, cls, pos, weight, bias, eps):
    """LN(cat(cls, patches) + pos) in float64 (HF CLIPVisionEmbeddings + pre_layrnorm)"""
    import torch
    x = vision_tokens(patches, cls, pos)
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), weight.double(), bias.double(), eps)


def text_tokens(ids, seq_len, tok, pos):
    """tok[clamp(ids[:, :seq_len], 0, vocab - 1)] + pos[:seq_len] in float32: one rounding per element, so any correct
    float32 evaluation gives these bits.  The clamp is the kernel's rule for an id outside the vocabulary."""
    idx = ids[:, :seq_len].clamp(0, tok.shape[0] - 1)
    return tok.float()[idx] + pos.float()[None, :seq_len, :]
