"""GPU: k-means on the device (lemon_amd/csrc/kmeans.hip, lemon_amd/kmeans.py) and the deep-kNN label score.

The assign kernel is held to the flat index bit for bit (that IS the reference's predict: index.search(x, 1)); update, split
and the train loop are held to tests/kmeans_ref.py, the float64 numpy restatement of the same rules."""
import os

import numpy as np
import pytest
import torch

from tests import kmeans_ref as R

pytestmark = pytest.mark.gpu


def _unit(rs, n, d):
    x = rs.randn(n, d).astype(np.float32)
    return x / np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)


def _case(n, C, d, unit_centroids, seed):
    """points (unit norm) and centroids with the awkward rows of the contract: exact duplicates among the centroids (the
    lower index must win) and points equal to a centroid (distance exactly 0)."""
    rs = np.random.RandomState(seed)
    x = _unit(rs, n, d)
    c = _unit(rs, C, d) if unit_centroids else (rs.randn(C, d) * rs.uniform(0.2, 3.0, (C, 1))).astype(np.float32)
    if C >= 4:
        c[C - 1] = c[1]                      # duplicate pair (1, C-1)
        c[C // 2] = c[0]                     # duplicate pair (0, C/2)
    for j in range(min(n, 3)):
        x[j] = c[(j * 7) % C]                # a point equal to a centroid
    return torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()


SHAPES = [(1, 1, 512), (1000, 100, 512), (40000, 100, 512), (5003, 1000, 768), (70000, 4096, 768),   # 4096 x 768 x 4 B = 12 MiB > LDS
          (777, 37, 1024), (513, 70, 36), (300, 5, 4)]


def _flat_search(x, c):
    from lemon_amd import IndexFlatL2
    idx = IndexFlatL2(c.shape[1], c.device)
    idx.add(c)
    D, I = idx.search(x, 1)
    return I[:, 0], D[:, 0]


@pytest.mark.parametrize("unit_centroids", [True, False])
@pytest.mark.parametrize("n,C,d", SHAPES)
def test_assign_equals_flat_search_bit_for_bit(hip, n, C, d, unit_centroids):
    from lemon_amd import kmeans
    x, c = _case(n, C, d, unit_centroids, seed=n + C)
    a = torch.full((n,), -7, dtype=torch.int32, device="cuda")            # poisoned outputs
    dist = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    kmeans.assign(x, c, out=(a, dist))
    I, D = _flat_search(x, c)
    assert torch.equal(a.to(torch.int64), I)
    assert torch.equal(dist.view(torch.int32), D.view(torch.int32))
    if C >= 4:                                # the planted rows: tie -> lower index, distance exactly 0
        for j in range(min(n, 3)):
            want = (j * 7) % C
            want = {C - 1: 1, C // 2: 0}.get(want, want)
            assert int(a[j]) == want and float(dist[j]) == 0.0


def test_assign_refuses_unsupported_shapes(hip):
    from lemon_amd import LemonHipError, kmeans
    x = torch.zeros((8, 1028), device="cuda")
    with pytest.raises(LemonHipError):
        kmeans.assign(x, x[:2].clone())                                    # d > 1024
    x = torch.zeros((8, 6), device="cuda")
    with pytest.raises(LemonHipError):
        kmeans.assign(x, x[:2].clone())                                    # d not a multiple of 4
    x = torch.zeros((16385, 8), device="cuda")
    with pytest.raises(LemonHipError):
        kmeans.assign(x, x.clone())                                        # C > 16384


@pytest.mark.parametrize("n,C,d", SHAPES)
def test_update_is_the_float64_mean_and_reproducible(hip, n, C, d):
    from lemon_amd import kmeans
    x, c = _case(n, C, d, True, seed=n + C)
    a, dist = kmeans.assign(x, c)
    c1 = c.clone()
    count, obj = kmeans.update(x, a, dist, c1)
    c2 = c.clone()
    count2, obj2 = kmeans.update(x, a, dist, c2)
    assert torch.equal(c1.view(torch.int32), c2.view(torch.int32)) and torch.equal(count, count2)
    assert torch.equal(obj.view(torch.int64), obj2.view(torch.int64))

    an = a.cpu().numpy().astype(np.int64)
    want_count = np.bincount(an, minlength=C)
    assert np.array_equal(count.cpu().numpy(), want_count) and want_count.sum() == n
    sums = torch.zeros((C, d), dtype=torch.float64).index_add_(0, torch.from_numpy(an), x.cpu().double()).numpy()
    got, old = c1.cpu().numpy(), c.cpu().numpy()
    full = want_count > 0
    ref32 = (sums[full] / want_count[full, None]).astype(np.float32)
    err = np.abs(got[full].astype(np.float64) - ref32.astype(np.float64))
    ulp = np.spacing(np.abs(ref32)).astype(np.float64)
    print(f"update ({n},{C},{d}): max error {float((err / ulp).max()):.3f} ulp")
    assert (err <= ulp).all()                 # one ulp: another float64 order can flip the final rounding
    assert np.array_equal(got[~full].view(np.int32), old[~full].view(np.int32))    # an empty cluster keeps its centroid
    if C >= 4:
        assert want_count[C - 1] == 0 and want_count[C // 2] == 0                  # the duplicates never win
    want_obj = dist.cpu().numpy().astype(np.float64).sum()
    rel = abs(float(obj[0]) - want_obj) / max(want_obj, 1e-300)
    print(f"update ({n},{C},{d}): obj relative error {rel:.3e}")
    assert rel <= 1e-12


def test_split_rule_matches_the_reference_exactly(hip):
    """two empty clusters (1 and 4) and a size tie (2 and 3): 1 takes half of 2 (the lower index of the tie), then 4 takes half
    of 3, the largest that is left"""
    from lemon_amd import kmeans
    rs = np.random.RandomState(5)
    c = rs.randn(6, 12).astype(np.float32)
    count = np.array([5, 0, 9, 9, 0, 3], np.int64)
    want_c, want_count = R.split_ref(c, count)
    assert want_count.tolist() == [5, 4, 5, 5, 4, 3]
    cd, nd = torch.from_numpy(c).cuda(), torch.from_numpy(count).cuda()
    kmeans.split_empty(cd, nd)
    assert np.array_equal(nd.cpu().numpy(), want_count)
    assert np.array_equal(cd.cpu().numpy().view(np.int32), want_c.view(np.int32))
    # nothing empty: nothing changes
    c2, n2 = torch.from_numpy(c).cuda(), torch.tensor([1, 2, 3, 4, 5, 6], device="cuda")
    kmeans.split_empty(c2, n2)
    assert np.array_equal(c2.cpu().numpy().view(np.int32), c.view(np.int32)) and n2.tolist() == [1, 2, 3, 4, 5, 6]


def _non_increasing(obj, rel=1e-6):
    return bool(np.all(obj[1:] <= obj[:-1] * (1.0 + rel) + 1e-300))


def test_train_on_planted_data_equals_float64_lloyd(hip):
    """tests/test_kmeans_host.py::test_planted_input_is_fair checks on the CPU that a float32 and the float64 numpy Lloyd
    agree exactly on this input, which is what makes "exactly" a fair demand here."""
    from lemon_amd import kmeans
    x, init_rows, truth = R.planted()
    niter = 6
    want_c, want_obj, want_count, want_a = R.lloyd_ref(x, x[init_rows], niter)
    xd = torch.from_numpy(x).cuda()
    c, obj, count, a = kmeans.train(xd, xd[torch.from_numpy(init_rows).cuda()], niter)
    assert np.array_equal(a.cpu().numpy().astype(np.int64), want_a)
    assert np.array_equal(want_a, truth)
    assert np.array_equal(count.cpu().numpy(), want_count)
    print("planted: max centroid difference", float(np.abs(c.cpu().numpy().astype(np.float64) - want_c).max()))
    assert np.abs(c.cpu().numpy().astype(np.float64) - want_c.astype(np.float64)).max() <= 1e-6
    obj = obj.cpu().numpy()
    assert _non_increasing(obj)
    # the float32 chain distance of one point is within (d + 3) 2^-24 (|x| + |c|)^2 of the exact one, norms below 1.2 here
    assert np.abs(obj - want_obj).max() <= len(x) * (x.shape[1] + 3) * 2.0 ** -24 * 2.4 ** 2


def test_train_on_random_unit_vectors(hip):
    """n = 20 000, C = 100, d = 512, niter = 25.  Points whose device assignment differs from a float64 assignment on the same
    centroids must be near-ties: float64 gap <= 2 (d + 3) 2^-24 (|x| + |c|)^2, the chain's worst-case rounding bound for the
    two distances compared (derived, not tuned), and at most 0.1 % of the points.  A float32 numpy assign on the centroids of
    a float32 numpy Lloyd of this input (tests/test_kmeans_host.py::test_float32_assign_stays_inside_the_cap) differs from
    the float64 one on 0 of the 20 000 points."""
    from lemon_amd import kmeans
    n, C, d, niter = 20000, 100, 512, 25
    rs = np.random.RandomState(11)
    x = _unit(rs, n, d)
    xd = torch.from_numpy(x).cuda()
    init = xd[torch.from_numpy(kmeans.initial_rows(n, C, 42, 0)).cuda()]
    c, obj, count, a = kmeans.train(xd, init, niter)
    obj = obj.cpu().numpy()
    assert _non_increasing(obj), obj
    count = count.cpu().numpy()
    assert count.sum() == n and (count > 0).all()
    a2 = kmeans.assign(xd, c, return_dist=False)
    assert torch.equal(a, a2)
    cn = c.cpu().numpy()
    d64 = R.sqdist(x, cn)
    a64 = d64.argmin(1)
    an = a.cpu().numpy().astype(np.int64)
    diff = np.flatnonzero(an != a64)
    print(f"random unit vectors: {len(diff)} of {n} assignments differ from float64")
    assert len(diff) <= n // 1000
    if len(diff):
        gap = d64[diff, an[diff]] - d64[diff, a64[diff]]
        cnorm = np.maximum(np.linalg.norm(cn[an[diff]].astype(np.float64), axis=1), np.linalg.norm(cn[a64[diff]].astype(np.float64), axis=1))
        cap = 2.0 * (d + 3) * 2.0 ** -24 * (np.linalg.norm(x[diff].astype(np.float64), axis=1) + cnorm) ** 2
        assert (gap <= cap).all(), (gap, cap)


def test_fit_is_reproducible_and_keeps_the_best_redo(hip):
    from lemon_amd import kmeans
    rs = np.random.RandomState(3)
    x = _unit(rs, 3000, 64)
    a = kmeans.KMeans(n_clusters=12, n_init=3, max_iter=15, seed=7).fit(x)
    b = kmeans.KMeans(n_clusters=12, n_init=3, max_iter=15, seed=7).fit(x)
    assert np.array_equal(a.cluster_centers_.view(np.int32), b.cluster_centers_.view(np.int32))
    assert np.array_equal(a.obj_, b.obj_) and a.inertia_ == b.inertia_ and a.best_redo_ == b.best_redo_
    assert a.cluster_centers_.shape == (12, 64) and a.cluster_centers_.dtype == np.float32
    finals = []
    xd = torch.from_numpy(x).cuda()
    for redo in range(3):
        init = xd[torch.from_numpy(kmeans.initial_rows(3000, 12, 7, redo)).cuda()]
        finals.append(float(kmeans.train(xd, init, 15)[1][-1]))
    assert a.best_redo_ == int(np.argmin(finals)) and a.inertia_ == min(finals)
    p = a.predict(x)
    assert p.shape == (3000, 1) and p.dtype == np.int64
    I, _ = _flat_search(xd, torch.from_numpy(a.cluster_centers_).cuda())
    assert np.array_equal(p[:, 0], I.cpu().numpy())


@pytest.mark.parametrize("data", ["planted", "random"])
def test_early_stop_cannot_change_the_result(hip, data, monkeypatch):
    """the device-side early stop (kernels behind the fixed point return at once) against LEMON_KMEANS_EARLY_STOP=0, which
    runs every iteration in full: equal bits.  The planted input reaches its fixed point in the second iteration, so 10 of
    its 12 iterations are skipped; the random one is still moving after 12."""
    from lemon_amd import kmeans
    if data == "planted":
        x, rows, _ = R.planted()
    else:
        x = _unit(np.random.RandomState(21), 6000, 128)
        rows = kmeans.initial_rows(6000, 40, 1, 0)
    xd = torch.from_numpy(x).cuda()
    init = xd[torch.from_numpy(rows).cuda()]
    monkeypatch.delenv("LEMON_KMEANS_EARLY_STOP", raising=False)
    fast = [t.cpu().numpy() for t in kmeans.train(xd, init, 12)]
    monkeypatch.setenv("LEMON_KMEANS_EARLY_STOP", "0")
    full = [t.cpu().numpy() for t in kmeans.train(xd, init, 12)]
    for a, b in zip(fast, full):
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
    if data == "planted":
        assert (fast[1][1:] == fast[1][1]).all()


def test_fit_subsamples_like_faiss(hip):
    from lemon_amd import kmeans
    rs = np.random.RandomState(9)
    x = _unit(rs, 3000, 32)
    km = kmeans.KMeans(n_clusters=2, n_init=1, max_iter=5, max_points_per_centroid=1024).fit(x)
    assert km.n_train_ == 2048
    rows = kmeans.subsample_rows(3000, 2, 1024, 42)
    want = R.lloyd_ref(x[rows], x[rows][kmeans.initial_rows(2048, 2, 42, 0)], 5)
    assert np.abs(km.cluster_centers_.astype(np.float64) - want[0]).max() <= 1e-5
    assert km.predict(x).shape == (3000, 1)


@pytest.mark.parametrize("drop_self", [False, True])
def test_label_disagreement_matches_numpy(hip, drop_self):
    from lemon_amd.baselines import label_disagreement
    rs = np.random.RandomState(2)
    nq, ntotal, k = 777, 500, 7
    kk = k + 1 if drop_self else k + 2
    I = rs.randint(0, ntotal, (nq, kk)).astype(np.int64)
    I[rs.rand(nq, kk) < 0.1] = -1                                          # padding slots
    db_label = rs.randint(-1, 6, ntotal).astype(np.int32)
    q_label = rs.randint(-1, 6, nq).astype(np.int32)
    in_db = (rs.rand(nq) < 0.5).astype(np.uint8)
    for mask in (None, in_db):
        got = label_disagreement(torch.from_numpy(I).cuda(), k, db_label, q_label, drop_self=drop_self, in_db=mask)
        want = R.label_disagreement_ref(I, k, db_label, q_label, drop_self, mask)
        assert np.array_equal(got.cpu().numpy(), want)
    assert (want[q_label < 0] == 1.0).all()


# ---- end to end: captions -> cluster labels -> deep-kNN score -> CLI ---------------------------------------------------
CLUSTERS = 20


@pytest.fixture(scope="module")
def clustered(hip):
    from lemon_amd import data
    kw = {"n_clusters": CLUSTERS, "clip_model": "huggingface_clip", "clip_path": "random"}     # seeded random ViT-B/32 towers
    return data.get_dataset("mscoco", 0, 0.4, "random", "synthetic:3000", cluster_text=True, cluster_kwargs=kw)


def test_cluster_text_labels_of_a_caption_dataset(hip, clustered):
    from lemon_amd import data
    plain = data.get_dataset("mscoco", 0, 0.4, "random", "synthetic:3000")
    km = clustered[0].cluster_model
    assert km.cluster_centers_.shape == (CLUSTERS, 512)
    for part, ref in zip(clustered, plain):
        assert len(part) == len(ref) > 0 and part.noisy_text == list(ref.noisy) and part.clean_text == list(ref.clean)
        assert part.noisy.dtype == np.int64 and part.clean.dtype == np.int64
        assert part.noisy.min() >= 0 and part.noisy.max() < CLUSTERS and part.clean.min() >= -1 and part.clean.max() < CLUSTERS
        mis = np.array([g != s for g, s in zip(ref.clean, ref.noisy)])
        assert 0 < mis.sum() < len(mis)
        assert np.array_equal(part.clean == -1, mis) and np.array_equal(part.clean[~mis], part.noisy[~mis])
        assert np.array_equal(part.noisy, km.predict(list(ref.noisy)).squeeze(1).cpu().numpy())     # val / test = km.predict
    assert len(np.unique(clustered[0].noisy)) > 1


@pytest.mark.parametrize("is_train", [False, True])
def test_deep_knn_scores_on_cluster_labels(hip, clustered, is_train):
    from lemon_amd import IndexFlatIP
    from lemon_amd.baselines import count_knn_distribution, deep_knn_scores
    train, val, _ = clustered
    rs = np.random.RandomState(4)
    e_tr = torch.from_numpy(_unit(rs, len(train), 64)).cuda()
    index = IndexFlatIP(64, e_tr.device)
    index.add(e_tr)
    k = 6
    if is_train:
        n_in = len(train) // 2                       # mixed in_db: the second half are "new" samples with train labels
        q = torch.cat([e_tr[:n_in], torch.from_numpy(_unit(rs, len(train) - n_in, 64)).cuda()])
        q_label, in_db = train.noisy, (np.arange(len(train)) < n_in).astype(np.uint8)
    else:
        q, q_label, in_db = torch.from_numpy(_unit(rs, len(val), 64)).cuda(), val.noisy, None
    got = deep_knn_scores(index, q, q_label, train.noisy, k, is_train=is_train, in_db=in_db).cpu().numpy()
    _, I = index.search(q, k + int(is_train))
    want = R.label_disagreement_ref(I.cpu().numpy(), k, train.noisy, q_label, is_train, in_db)
    assert np.array_equal(got, want) and got.min() >= 0.0 and got.max() <= 1.0
    # the label-based kNN statistic the project already ships takes the cluster ids as they are
    dist = count_knn_distribution(CLUSTERS, 0.0, e_tr, train.noisy, k)
    assert dist.shape == (len(train), CLUSTERS) and bool(torch.isfinite(dist).all())


def test_deepknn_cli_on_synthetic_captions(hip, tmp_path):
    from lemon_amd import data
    from lemon_amd.deepknn_baseline import main
    out = str(tmp_path / "deepknn")
    rc = main(["--output_dir", out, "--dataset", "mscoco", "--flip_type", "random", "--percent_flips", "0.4", "--noise_labels",
               "--data_root", "synthetic:3000", "--clip_path", "random", "--num_text_clusters", str(CLUSTERS), "--knn_k", "5",
               "--debug"])
    assert rc == 0
    for f in ("dists.npy", "label_flips_all.npy", "datasplit.npy", "len_splits.npy", "runtime.npy", "args.json", "done"):
        assert os.path.exists(os.path.join(out, f)), f
    sets = data.get_dataset("mscoco", 0, 0.4, "random", "synthetic:3000")
    n = [len(s) for s in sets]                       # train, val, test
    dists, flips, split = (np.load(os.path.join(out, f)) for f in ("dists.npy", "label_flips_all.npy", "datasplit.npy"))
    assert dists.shape == flips.shape == split.shape == (sum(n),) and dists.dtype == np.float32
    assert split.tolist() == ["train"] * n[0] + ["test"] * n[2] + ["val"] * n[1]
    assert np.isin(np.round(dists * 5), np.arange(6)).all()
    assert np.load(os.path.join(out, "len_splits.npy")).tolist() == [(m + 257) // 258 for m in (n[0], n[2], n[1])]
    gold = np.concatenate([[g != s for g, s in zip(p.clean, p.noisy)] for p in (sets[0], sets[2], sets[1])])
    assert np.array_equal(flips.astype(bool), gold)
