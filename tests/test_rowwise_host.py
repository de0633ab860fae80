"""CPU: tests/rowwise_ref.py -- the float64 references tests/test_gpu_rowwise.py holds the row-wise and token kernels to --
against sklearn, scipy and torch.nn.functional in float64, against the two recorded fixtures (tests/golden/zero_shot.npz,
written by the reference's own code, and the CPU oracle's d1_normalized / paired_distance / score), and the error brackets
against float32 evaluations in several summation orders.  No GPU."""
import os

import numpy as np
import pytest
import torch

from tests import rowwise_ref as R
from tests.synth import planted

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _rows(rng, n, d, scale=1.0):
    return (rng.standard_normal((n, d)) * scale).astype(np.float32)


def test_normalize_rows_is_torch_normalize_in_float64():
    rng = np.random.default_rng(0)
    x = _rows(rng, 9, 260, 3.0)
    x[2] = 0.0
    x[3] = 1e-20
    x[4] = 1e30
    x[5, 7] = 1e-40
    ref = torch.nn.functional.normalize(torch.from_numpy(x).double(), p=2.0, dim=1, eps=1e-12).numpy()
    got = R.normalize_rows(x)
    assert np.allclose(got, ref, rtol=1e-15, atol=0.0)
    assert np.all(got[2] == 0.0) and np.allclose(got[3], 1e-8, rtol=1e-6)       # below the floor: divided by 1e-12
    assert np.allclose(np.linalg.norm(got[[0, 1, 4, 5]], axis=1), 1.0, rtol=1e-14)


def test_ulps_counts_float32_spacings():
    ref = np.array([1.0, 1.0, 3e-45, 0.0, 2.0])
    got = np.array([1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 0.0, 0.0, np.nan], np.float32)
    e = R.ulps(got, ref)
    assert e[0] == 1.0 and e[1] == 0.5 and e[3] == 0.0 and e[4] == np.inf
    assert e[2] == pytest.approx(2.0)             # 3e-45 rounds to two subnormal steps


@pytest.mark.parametrize("d", [1, 63, 129])
def test_paired_metrics_are_sklearn_diagonals_in_float64(d):
    from sklearn.metrics.pairwise import cosine_similarity, euclidean_distances, manhattan_distances
    rng = np.random.default_rng(d)
    a, b = _rows(rng, 65, d, 3.0).astype(np.float64), _rows(rng, 65, d, 0.5).astype(np.float64)
    a[3] = 0.0                                     # sklearn: a zero row has similarity 0, distance 1
    b[5] = 0.0
    a[7] = b[7]
    assert np.allclose(R.paired(5, a, b), 1 - np.diagonal(cosine_similarity(a, b)), rtol=0, atol=1e-14)
    assert R.paired(5, a, b)[3] == 1.0 and R.paired(5, a, b)[5] == 1.0 and abs(R.paired(5, a, b)[7]) < 1e-15
    # (sklearn's float64 euclidean goes through |a|^2 + |b|^2 - 2 <a, b>: absolute error ~ 1e-16 |a|^2 / dist)
    far = np.arange(65) != 7
    assert np.allclose(R.paired(3, a, b)[far], np.diagonal(euclidean_distances(a, b))[far], rtol=1e-11, atol=0)
    assert R.paired(3, a, b)[7] == 0.0 and R.paired(4, a, b)[7] == 0.0
    assert np.allclose(R.paired(4, a, b), np.diagonal(manhattan_distances(a, b)), rtol=1e-14, atol=0)
    assert np.allclose(R.paired(2, a, b), R.paired(3, a, b) ** 2, rtol=1e-14, atol=0)
    assert np.allclose(R.paired(1, a, b), 1 - np.einsum("ij,ij->i", a, b), rtol=0, atol=1e-13)
    # scale invariance of the cosine, the property the GPU test asks of the kernel
    assert np.allclose(R.paired(5, 1e-10 * a, 1e10 * b), R.paired(5, a, b), rtol=0, atol=1e-14)


def _f32_sum(terms, parts):
    """float32 sum of terms [n, d] in `parts` interleaved partial chains, added pairwise at the end"""
    acc = np.zeros((terms.shape[0], parts), np.float32)
    for k in range(terms.shape[1]):
        acc[:, k % parts] = acc[:, k % parts] + terms[:, k]
    while acc.shape[1] > 1:
        acc = acc[:, 0::2] + acc[:, 1::2]
    return acc[:, 0]


@pytest.mark.parametrize("parts", [1, 4])
@pytest.mark.parametrize("d", [1, 65, 512])
def test_chain_bound_holds_for_float32_sums_in_any_order(d, parts):
    rng = np.random.default_rng(7 * d + parts)
    a, b = _rows(rng, 40, d, 3.0), _rows(rng, 40, d, 0.5)
    one = np.float32(1.0)
    dif = a - b
    got = {1: one - _f32_sum(a * b, parts), 2: _f32_sum(dif * dif, parts), 3: np.sqrt(_f32_sum(dif * dif, parts)),
           4: _f32_sum(np.abs(dif), parts),
           5: one - _f32_sum(a * b, parts) / (np.sqrt(_f32_sum(a * a, parts)) * np.sqrt(_f32_sum(b * b, parts)))}
    for mode, g in got.items():
        err = np.abs(g.astype(np.float64) - R.paired(mode, a, b))
        bound = R.paired_chain_bound(mode, a, b)
        assert np.all(err <= bound), (mode, float((err / bound).max()))
        # ... and is no blank cheque: dropping the last term of every row breaks it (d > 1)
        if d > 1 and mode in (2, 4):
            short = R.paired(mode, a[:, :-1], b[:, :-1])
            assert np.any(np.abs(short - R.paired(mode, a, b)) > bound)


def test_single_chain_at_d512_misses_the_reference_bar_and_float64_sums_meet_it():
    # the finding behind the kernels' float64 sums: |rows| ~ 10, d = 512 (raw CLIP embeddings)
    rng = np.random.default_rng(3)
    a, b = _rows(rng, 64, 512, 10 / 512 ** 0.5), _rows(rng, 64, 512, 10 / 512 ** 0.5)
    for mode, terms in ((4, np.abs(a - b)), (3, (a - b) * (a - b))):
        ref = R.paired(mode, a, b)
        e32 = np.abs(R.sk_paired_metric(R.KIND_OF_MODE[mode], a, b).astype(np.float64) - ref).max()
        bar = R.reference_bar(e32, np.abs(ref))
        chain = _f32_sum(terms, 1)
        chain = np.sqrt(chain) if mode == 3 else chain
        assert np.any(np.abs(chain.astype(np.float64) - ref) > bar), mode
        wide = ref.astype(np.float32)                      # float64 sums, one rounding
        assert np.all(np.abs(wide.astype(np.float64) - ref) <= bar), mode


def test_class_distances_and_softmax_against_sklearn_and_scipy():
    from scipy.special import softmax
    from sklearn.metrics.pairwise import cosine_similarity, euclidean_distances, manhattan_distances
    rng = np.random.default_rng(1)
    img, cls = _rows(rng, 5, 24, 2.0).astype(np.float64), _rows(rng, 65, 24, 0.7).astype(np.float64)
    img[1] = 0.0
    cls[64] = 0.0
    assert np.allclose(R.class_distances(0, img, cls), 1 - cosine_similarity(img, cls), rtol=0, atol=1e-14)
    assert np.all(R.class_distances(0, img, cls)[1] == 1.0) and np.all(R.class_distances(0, img, cls)[:, 64] == 1.0)
    assert np.allclose(R.class_distances(1, img, cls), euclidean_distances(img, cls), rtol=1e-11, atol=0)
    assert np.allclose(R.class_distances(2, img, cls), manhattan_distances(img, cls), rtol=1e-14, atol=0)
    assert np.allclose(R.class_distances("l2", img, cls), euclidean_distances(img, cls, squared=True), rtol=1e-11, atol=0)
    assert np.allclose(R.class_distances("ip", img, cls), 1 - img @ cls.T, rtol=0, atol=1e-14)
    z = rng.standard_normal((5, 65)) * 30
    assert np.allclose(R.softmax_rows(z), softmax(z, axis=1), rtol=1e-13, atol=0)
    lab = np.array([0, 64, 63, 1, 7])
    for kind in (0, 1, 2):
        ref = softmax(1 - R.class_distances(kind, img, cls), axis=1)[np.arange(5), lab]
        assert np.allclose(R.class_confidence(kind, img, cls, lab), ref, rtol=1e-13, atol=0)
        # the float32 route of the reference project agrees with it to float32 accuracy
        assert np.allclose(R.sk_class_confidence(kind, img, cls, lab), ref, rtol=2e-5, atol=0)
    assert np.allclose(R.class_confidence(0, img, cls, lab)[1], 1 / 65, rtol=1e-14)      # a zero image: every class at distance 1


def test_labels_outside_the_classes_raise_or_wrap_like_numpy():
    rng = np.random.default_rng(2)
    img, cls = _rows(rng, 3, 8), _rows(rng, 10, 8)
    with pytest.raises(IndexError):
        R.class_confidence(0, img, cls, [0, 10, 1])
    with pytest.raises(IndexError):
        R.d1_normalized("ip", img, cls, [0, 1, 1025])
    assert np.array_equal(R.d1_normalized("l2", img, cls, [-1, -10, 3]), R.d1_normalized("l2", img, cls, [9, 0, 3]))


def test_checked_labels_raises_before_anything_is_uploaded():
    from lemon_amd.ops import checked_labels
    ok = checked_labels(np.array([0, 9, 3]), 3, 10, "cpu")
    assert ok.dtype == torch.int32 and ok.tolist() == [0, 9, 3]
    assert checked_labels(torch.tensor([4], dtype=torch.int64), 1, 5, "cpu").tolist() == [4]
    assert checked_labels([], 0, 5, "cpu").numel() == 0
    for bad in ([0, 10, 1], [0, -1, 1], [2 ** 31, 0, 0]):
        with pytest.raises(ValueError):
            checked_labels(np.array(bad), 3, 10, "cpu")
    with pytest.raises(ValueError):
        checked_labels(np.array([0, 1]), 3, 10, "cpu")                  # one label per row
    with pytest.raises(ValueError):
        checked_labels(np.array([0.0, 1.0, 2.0]), 3, 10, "cpu")


@pytest.mark.parametrize("dist", R.KIND_NAMES)
def test_class_confidence_matches_the_reference_golden(dist):
    g = np.load(os.path.join(GOLDEN, "zero_shot.npz"))
    kind = R.KIND_NAMES.index(dist)
    ref = R.class_confidence(kind, g["img"], g["cls"], g["lab"])
    assert np.abs(ref - g[f"conf_{dist}"]).max() <= 2e-6
    # the reference's route re-run here lands on the recording to float32 accuracy as well
    again = R.sk_class_confidence(kind, g["img"], g["cls"], g["lab"])
    assert np.abs(again - g[f"conf_{dist}"]).max() <= 2e-6


def test_d1_normalized_and_its_bound_against_the_oracle(oracle):
    s = planted(seed=4, n_tr=10, n_q=300, d=64, C=100)
    q_img, _, _, noisy = s["query"]
    for metric, name in (("ip", "cosine"), ("l2", "euclidean")):
        ref = R.d1_normalized(metric, q_img, s["proto"], noisy)
        got = oracle.d1_normalized(name, q_img, s["proto"], noisy).astype(np.float64)
        assert np.abs(got - ref).max() <= 1e-6
        rel = np.abs(got - ref) / ref
        assert np.all(rel <= R.d1_chain_bound(metric, q_img, s["proto"])), float((rel / R.d1_chain_bound(metric, q_img, s["proto"])).max())
    assert np.allclose(R.softmax_rows(R.class_distances("ip", q_img, s["proto"])).sum(1), 1.0, rtol=1e-14)


def test_paired_modes_1_2_against_the_oracle_chain(oracle):
    rng = np.random.default_rng(5)
    for d in (1, 65, 512):
        a, b = _rows(rng, 33, d), _rows(rng, 33, d)
        for mode, name in ((1, "cosine"), (2, "euclidean")):
            got = oracle.paired_distance(name, a, b).astype(np.float64)
            assert np.all(np.abs(got - R.paired(mode, a, b)) <= R.paired_chain_bound(mode, a, b)), (mode, d)


def test_score_against_the_oracle_and_at_its_edges(oracle):
    rng = np.random.default_rng(6)
    n, k = 37, 5
    rec = {"d_1": rng.random(n).astype(np.float32)}
    for nm in ("D_n", "dists_tr_n", "dists_n", "D_m", "dists_tr_m", "dists_m"):
        rec[nm] = (0.0625 + rng.random((n, k))).astype(np.float32)
    hp = dict(beta=5.0, gamma=3.0, tau_1_n=0.1, tau_2_n=5.0, tau_1_m=1.5, tau_2_m=0.0)
    s, dn, dm = R.score(rec, hp)
    so, dno, dmo = oracle.score(rec, hp, return_dn=True)
    assert np.allclose(s, so, rtol=1e-9, atol=0) and np.allclose(dn, dno, rtol=1e-9, atol=0) and np.allclose(dm, dmo, rtol=1e-9, atol=0)
    # every tau zero: the mean of dists_*, exactly (the float32 values sum without rounding in float64)
    s0, dn0, dm0 = R.score(rec, [2.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    assert np.array_equal(dn0, rec["dists_n"].astype(np.float64).sum(1) / k) and np.array_equal(dn0, oracle.score(rec, dict(zip(R.HP_ORDER, [2.0, 0, 0, 0, 0, 0])), True)[1])
    # weights that underflow: the score is d_1
    s1, _, _ = R.score(rec, [5.0, 3.0, 1e6, 0.0, 1e6, 0.0])
    assert np.array_equal(s1, rec["d_1"].astype(np.float64))
    # inf x 0 = NaN where dists is zero, inf elsewhere
    rec2 = {key: v.copy() for key, v in rec.items()}
    rec2["D_n"] = -rec2["D_n"]
    rec2["dists_n"][::3, 2] = 0.0
    s2, dn2, _ = R.score(rec2, [5.0, 3.0, 1e6, 0.0, 0.1, 0.0])
    assert np.isnan(dn2[::3]).all() and np.isinf(np.delete(dn2, np.arange(0, n, 3))).all()
    assert np.array_equal(s2, oracle.score(rec2, dict(zip(R.HP_ORDER, [5.0, 3.0, 1e6, 0.0, 0.1, 0.0]))), equal_nan=True)


def test_token_references_against_torch_functional():
    g = torch.Generator().manual_seed(0)
    B, T, W = 3, 5, 36
    patches, cls, pos = torch.randn(B, T - 1, W, generator=g), torch.randn(W, generator=g), torch.randn(T, W, generator=g)
    w, b = 1 + 0.3 * torch.randn(W, generator=g), 0.2 * torch.randn(W, generator=g)
    x = R.vision_tokens(patches, cls, pos)
    assert x.dtype == torch.float64 and torch.equal(x[1, 0], cls.double() + pos[0].double()) and torch.equal(x[2, 3], patches[2, 2].double() + pos[3].double())
    mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    manual = (x - mean) / torch.sqrt(var + 1e-5) * w.double() + b.double()
    assert torch.allclose(R.vision_tokens_ln(patches, cls, pos, w, b, 1e-5), manual, rtol=1e-12, atol=1e-13)
    vocab = 50
    tok, tpos = torch.randn(vocab, W, generator=g), torch.randn(7, W, generator=g)
    ids = torch.randint(0, vocab, (B, 12), generator=g)
    ids[:, 7:] = 2 ** 40
    ref = torch.nn.functional.embedding(ids[:, :7], tok) + tpos[None]
    assert torch.equal(R.text_tokens(ids, 7, tok, tpos), ref)
    ids[0, 0], ids[1, 1], ids[2, 2], ids[0, 3] = 0, vocab - 1, -3, vocab + 9
    y = R.text_tokens(ids, 7, tok, tpos)
    assert torch.equal(y[2, 2], tok[0] + tpos[2]) and torch.equal(y[0, 3], tok[vocab - 1] + tpos[3])
