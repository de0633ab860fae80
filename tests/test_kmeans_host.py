"""CPU: the host side of lemon_amd.kmeans (sub-sample / seed / redo rules against tests/kmeans_ref.py with the device calls
stubbed), the fairness checks the GPU tests rely on, get_dataset's unchanged default, the deep-kNN CLI's argument surface,
the C-ABI entries and the build of the new translation unit."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import kmeans_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["lemon_kmeans_assign", "lemon_kmeans_update", "lemon_kmeans_split", "lemon_kmeans_train",
               "lemon_kmeans_workspace_bytes", "lemon_knn_label_disagreement"]


@pytest.fixture
def stubbed(monkeypatch):
    """lemon_amd.kmeans with train / assign replaced by the numpy reference on CPU tensors; records every train call."""
    from lemon_amd import kmeans
    calls = []

    def train(x, init, niter):
        xn, cn = x.numpy(), init.numpy()
        calls.append((xn.copy(), cn.copy(), niter))
        c, obj, count, a = R.lloyd_ref(xn, cn, niter)
        return torch.from_numpy(c), torch.from_numpy(obj), torch.from_numpy(count), torch.from_numpy(a.astype(np.int32))

    def assign(x, c, return_dist=True, out=None):
        a, dist = R.assign_ref(x.numpy(), c.numpy())
        a = torch.from_numpy(a.astype(np.int32))
        return (a, torch.from_numpy(dist.astype(np.float32))) if return_dist else a

    monkeypatch.setattr(kmeans, "train", train)
    monkeypatch.setattr(kmeans, "assign", assign)
    return kmeans, calls


def _blobs(n, d, C, seed):
    rs = np.random.RandomState(seed)
    centres = rs.randn(C, d) * 3
    return (centres[rs.randint(0, C, n)] + rs.randn(n, d)).astype(np.float32)


def test_seed_and_permutation_rules(stubbed):
    kmeans, calls = stubbed
    x = _blobs(400, 8, 5, 0)
    km = kmeans.KMeans(n_clusters=5, n_init=3, max_iter=4, seed=42, device="cpu").fit(x)
    assert len(calls) == 3 and km.n_train_ == 400
    for redo, (xn, init, niter) in enumerate(calls):
        assert niter == 4 and np.array_equal(xn, x)
        rows = np.random.RandomState(42 + redo).permutation(400)[:5]
        assert np.array_equal(init, x[rows])
    # another seed starts elsewhere
    assert not np.array_equal(kmeans.initial_rows(400, 5, 43, 0), kmeans.initial_rows(400, 5, 42, 0))
    assert np.array_equal(kmeans.initial_rows(400, 5, 43, 0), kmeans.initial_rows(400, 5, 42, 1))


def test_best_redo_is_kept_and_ties_go_to_the_earlier(stubbed):
    kmeans, calls = stubbed
    x = _blobs(600, 8, 7, 1)
    km = kmeans.KMeans(n_clusters=7, n_init=4, max_iter=6, seed=3, device="cpu").fit(x)
    finals = [R.lloyd_ref(x, x[kmeans.initial_rows(600, 7, 3, r)], 6) for r in range(4)]
    objs = [f[1][-1] for f in finals]
    best = int(np.argmin(objs))                  # np.argmin: the first minimum = the earlier redo
    assert km.best_redo_ == best and km.inertia_ == objs[best]
    assert np.array_equal(km.obj_, finals[best][1])
    assert np.array_equal(km.cluster_centers_, finals[best][0]) and km.cluster_centers_.dtype == np.float32
    p = km.predict(x)
    assert p.shape == (600, 1) and p.dtype == np.int64 and np.array_equal(p[:, 0], finals[best][3])
    # identical redos (n_clusters == n: every permutation head is the whole set, objective 0): the first one is kept
    y = _blobs(4, 4, 4, 2)
    assert kmeans.KMeans(n_clusters=4, n_init=3, max_iter=2, device="cpu").fit(y).best_redo_ == 0


def test_subsample_rule(stubbed):
    kmeans, calls = stubbed
    x = _blobs(3000, 4, 2, 4)
    km = kmeans.KMeans(n_clusters=2, n_init=1, max_iter=2, max_points_per_centroid=1024, seed=42, device="cpu").fit(x)
    rows = np.random.RandomState(42).permutation(3000)[:2048]
    assert km.n_train_ == 2048 and len(set(rows.tolist())) == 2048
    assert np.array_equal(calls[0][0], x[rows])
    assert np.array_equal(calls[0][1], x[rows][np.random.RandomState(42).permutation(2048)[:2]])
    assert km.predict(x).shape == (3000, 1)
    assert kmeans.subsample_rows(2048, 2, 1024, 42) is None          # n == cap: everything is used


def test_predict_on_strings_goes_through_embed_func(stubbed):
    kmeans, _ = stubbed
    x = _blobs(50, 4, 3, 5)
    km = kmeans.KMeans(n_clusters=3, n_init=1, max_iter=3, device="cpu", embed_func=lambda texts: x[[int(t) for t in texts]])
    km.fit(x)
    assert np.array_equal(km.predict(["3", "7"]), km.predict(x[[3, 7]]))
    with pytest.raises(TypeError):
        kmeans.KMeans(n_clusters=3, device="cpu").predict(["a"])
    with pytest.raises(ValueError):
        kmeans.KMeans(n_clusters=0)
    with pytest.raises(ValueError):
        kmeans.KMeans(n_clusters=3, device="cpu").fit(x[:2])


def test_planted_input_is_fair():
    """a float32 and the float64 numpy Lloyd agree exactly on the planted input of the GPU test: rounding cannot move a point"""
    x, rows, truth = R.planted()
    a = R.lloyd_ref(x, x[rows], 6, np.float64)
    b = R.lloyd_ref(x, x[rows], 6, np.float32)
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[3], truth)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[2], b[2])
    assert np.all(a[1][1:] <= a[1][:-1] * (1 + 1e-6))


def test_float32_assign_stays_inside_the_cap():
    """the input of test_gpu_kmeans.py::test_train_on_random_unit_vectors: a float32 numpy assign differs from the float64 one
    only on near-ties below the chain's rounding bound (count observed: 0 of 20 000)"""
    from lemon_amd import kmeans
    n, C, d, niter = 20000, 100, 512, 25
    rs = np.random.RandomState(11)
    x = rs.randn(n, d).astype(np.float32)
    x = x / np.linalg.norm(x, axis=1, keepdims=True).astype(np.float32)
    c, obj, count, a32 = R.lloyd_ref(x, x[kmeans.initial_rows(n, C, 42, 0)], niter, np.float32)
    assert np.all(obj[1:] <= obj[:-1] * (1 + 1e-6)) and count.sum() == n and (count > 0).all()
    d64 = R.sqdist(x, c)
    a64 = d64.argmin(1)
    diff = np.flatnonzero(a32 != a64)
    print(f"float32 numpy assign differs from float64 on {len(diff)} of {n} points")
    assert len(diff) <= n // 1000
    gap = d64[diff, a32[diff]] - d64[diff, a64[diff]]
    cnorm = np.maximum(np.linalg.norm(c[a32[diff]], axis=1), np.linalg.norm(c[a64[diff]], axis=1))
    assert (gap <= 2.0 * (d + 3) * 2.0 ** -24 * (1.0 + cnorm) ** 2).all()


def test_split_reference_rule():
    c = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    out, count = R.split_ref(c, np.array([0, 7, 2]))
    assert count.tolist() == [3, 4, 2]
    assert np.array_equal(out[0], c[1] * np.float32([1 + R.EPS, 1 - R.EPS] * 2))
    assert np.array_equal(out[1], c[1] * np.float32([1 - R.EPS, 1 + R.EPS] * 2))
    assert np.array_equal(out[2], c[2])


def test_get_dataset_default_is_unchanged():
    from lemon_amd import data
    sig = inspect.signature(data.get_dataset)
    assert sig.parameters["cluster_text"].default is False and sig.parameters["cluster_kwargs"].default is None
    a = data.get_dataset("mscoco", 0, 0.4, "random", "synthetic:400")
    b = data.get_dataset("mscoco", 0, 0.4, "random", "synthetic:400", cluster_text=False, cluster_kwargs=None)
    for sa, sb in zip(a, b):
        assert sa.noisy == sb.noisy and sa.clean == sb.clean and np.array_equal(sa.images, sb.images)
        assert isinstance(sa.noisy[0], str)
    # class datasets ignore the flag, as upstream (no text tower is built: cluster_kwargs may be empty)
    a = data.get_dataset("cifar10", 0, 0.4, "symmetric", "synthetic:200")
    b = data.get_dataset("cifar10", 0, 0.4, "symmetric", "synthetic:200", cluster_text=True, cluster_kwargs={})
    for sa, sb in zip(a, b):
        assert np.array_equal(sa.noisy, sb.noisy) and np.array_equal(sa.clean, sb.clean)
    with pytest.raises(ValueError):
        data.get_dataset("mscoco", 0, 0.4, "random", "synthetic:400", cluster_text=True, cluster_kwargs={"n_clusters": 5})


def test_deepknn_cli_surface():
    from lemon_amd.deepknn_baseline import build_parser, check_defined
    p = build_parser()
    a = p.parse_args(["--output_dir", "o", "--noise_labels"])
    want = dict(dataset="cifar10", algorithm="huggingface_clip", seed=0, flip_type="real", batch_size=258, percent_flips=0.3,
                dist_type="cosine", val_only=False, knn_k=10, num_text_clusters=100, agg_type="mean", dist_method="deep_knn",
                deep_knn_thres=0.5, data_root="./data", clip_path="random")
    for k, v in want.items():
        assert getattr(a, k) == v, k
    check_defined(a)
    assert p.parse_args(["--output_dir", "o", "--data_dir", "/x"]).data_root == "/x"
    assert p.parse_args(["--output_dir", "o", "--data_root", "synthetic:9"]).data_root == "synthetic:9"
    for flag, val in (("--agg_type", "max"), ("--dist_method", "nn_ot"), ("--deep_knn_thres", "0.7")):
        with pytest.raises(NotImplementedError, match=flag[2:]):
            check_defined(p.parse_args(["--output_dir", "o", "--noise_labels", flag, val]))
    with pytest.raises(NotImplementedError):
        check_defined(p.parse_args(["--output_dir", "o"]))                 # run_deepknn.py:245-246
    with pytest.raises(SystemExit):
        p.parse_args(["--output_dir", "o", "--dist_method", "invented"])


def test_header_and_exports_carry_the_new_entries():
    from lemon_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lemon_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lemon_[a-z0-9_]+)\s*\(", hdr))
    lib = ctypes.CDLL(_lib.SO_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTS and hasattr(lib, name), name


def test_library_is_built_from_the_new_translation_unit():
    from lemon_amd import _lib, build
    assert "kmeans.hip" in build.SOURCES
    blob = open(_lib.SO_PATH, "rb").read()
    assert b"gfx950" in blob and b"k_kmeans_assign" in blob


def test_kmeans_kernels_do_not_spill():
    from tests.test_build_guard import HIPCC, _kernel_meta
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    meta = _kernel_meta("kmeans.hip")
    for frag in ("k_kmeans_assign", "k_km_keys", "k_km_bounds", "k_km_means", "k_km_obj", "k_km_split", "k_label_disagreement"):
        hits = [n for n in meta if frag in n]
        assert hits, frag
        for n in hits:
            assert meta[n]["vgpr_spill_count"] == 0 and meta[n]["private_segment_fixed_size"] == 0, (n, meta[n])
            if "k_kmeans_assign" in n:
                assert meta[n]["vgpr_count"] <= 256, (n, meta[n])      # two workgroups per CU


def test_label_disagreement_reference():
    I = np.array([[0, 1, 2, -1], [3, 0, 1, 2]])
    db = np.array([5, 5, 6, -1], np.int32)
    q = np.array([5, -1], np.int32)
    assert R.label_disagreement_ref(I, 3, db, q).tolist() == [np.float32(1) / np.float32(3), 1.0]
    assert R.label_disagreement_ref(I, 3, db, q, True, np.array([1, 0])).tolist() == [np.float32(2) / np.float32(3), 1.0]
