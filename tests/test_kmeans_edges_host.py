"""CPU: the inputs of tests/test_gpu_kmeans_edges.py are fair and reach the edges they are meant for (tests/kmeansfx.py), and
KMeans.fit refuses non-finite input before it launches anything.  What the GPU tests demand exactly is shown here to survive
float32 rounding in a plain numpy restatement (tests/kmeans_ref.py)."""
import numpy as np
import pytest
import torch

from tests import kmeans_ref as R
from tests import kmeansfx as F
from tests.test_kmeans_host import stubbed  # noqa: F401  (fixture)


def test_assign_shapes_cover_every_value_and_the_required_combinations():
    shapes = F.assign_shapes()
    assert 55 <= len(shapes) <= 65 and len(set(shapes)) == len(shapes)
    assert {s[0] for s in shapes} == set(F.ASSIGN_N)
    assert {s[1] for s in shapes} == set(F.ASSIGN_C)
    assert {s[2] for s in shapes} == set(F.ASSIGN_D)
    pairs = {(C, d) for _, C, d in shapes}
    for d in (4, 28, 32):                        # one k-slice, several centroid tiles
        for C in (129, 257):
            assert (C, d) in pairs
    assert (129, 1024) in pairs
    assert (129, 16384, 4) in shapes and (129, 16384, 36) in shapes


@pytest.mark.parametrize("unit_centroids", [True, False])
def test_float32_numpy_assign_stays_inside_the_cap_on_the_assign_inputs(unit_centroids):
    """a float32 numpy assign on every input of the GPU test passes the GPU test's float64 checks (count observed: 0 points
    differ on every case), so the cap of n // 1000 -- no point at all at these n -- is a fair demand"""
    total = 0
    for n, C, d in F.assign_shapes():
        x, c = F.assign_case(n, C, d, unit_centroids)
        assert len(np.unique(c, axis=0)) == (C - 2 if C >= 8 else C)       # the two planted pairs and no other duplicate
        a32, d32 = R.assign_ref(x, c, np.float32)
        total += F.check_against_float64(x, c, a32)
    print(f"float32 numpy assign differs from float64 on {total} points over all cases")


def test_tie_table_reaches_every_merge_path():
    kinds = set()
    for pair in F.TIE_PAIRS:
        for d in (8, 36):
            x, c, lo, hi = F.tie_case(pair, d)
            assert (lo, hi) == (min(pair), max(pair)) and len(x) == 201 and c.shape == (F.TIE_C, d)
            assert np.array_equal(c[lo].view(np.int32), c[hi].view(np.int32)) and np.array_equal(x[0], c[lo])
            assert len(np.unique(c, axis=0)) == F.TIE_C - 1                # no duplicate beyond the pair
            # the pair is the nearest centroid of many points, and float64 gives the lower index
            a64 = R.sqdist(x, c).argmin(1)
            assert (a64 == lo).sum() >= 50 and not (a64 == hi).any()
        lo, hi = min(pair), max(pair)
        if lo // 128 != hi // 128:
            kinds.add("tile")
        elif lo // 32 != hi // 32:
            kinds.add("group")
        if F.lane_half(lo) == F.lane_half(hi):
            kinds.add("same half")
        else:
            kinds.add("lower index in the upper half" if F.lane_half(lo) else "lower index in the lower half")
    assert kinds == {"tile", "group", "same half", "lower index in the upper half", "lower index in the lower half"}
    assert F.TIE_PAIRS[-1] == (12, 9)            # written at 12 first: the copy has the lower index


def test_crafted_assignments_have_the_sizes_they_claim():
    for n, C, d, pattern in F.UPDATE_CASES:
        assert n <= 5000
        a = F.crafted_assign(n, C, pattern)
        assert a.dtype == np.int32 and a.shape == (n,)
        ok = (a >= 0) & (a < C)
        count = np.bincount(a[ok], minlength=C)
        if pattern == "all":
            assert count.max() == n
        elif pattern == "none":
            assert not ok.any() and set(a.tolist()) <= {-1, C, 2 ** 31 - 1}
        else:
            assert {-1, C, 2 ** 31 - 1} <= set(a.tolist()) and (~ok).sum() == 30
        if pattern == "sizes":
            assert set(F.UPDATE_SIZES) <= set(count.tolist()) and count[0] == 1 and count[C - 1] == 9
            assert (count > 0).sum() == 8        # seven small clusters and the large one; the rest is empty
    assert {c[1] for c in F.UPDATE_CASES} == {1, 255, 256, 257, 16384}
    assert {c[2] for c in F.UPDATE_CASES} == {4, 36, 128, 132, 1024}
    assert {n for n, C, _, _ in F.UPDATE_CASES if C >= 255 and n != 300} == {5000}


def test_split_patterns_reach_the_reduction_edges():
    cases = F.split_cases()
    assert {c[0] for c in cases} == set(F.SPLIT_C) and {c[1] for c in cases} == {4, 36, 1024}
    assert max(C for C, d, _ in cases if d == 1024) == 4097
    for C in F.SPLIT_C:
        assert {p for cc, _, p in cases if cc == C} == set(F.SPLIT_PATTERNS)
    for C in (1025, 16384):
        count = F.split_counts(C, "equal")
        full = np.flatnonzero(count)
        assert set(count.tolist()) == {0, 5} and len({int(i) // 64 % 16 for i in full}) == 16      # the tie spans every wave
        c = np.ones((C, 4), np.float32)
        _, after = R.split_ref(c, count)
        assert after.sum() == count.sum() and after[full[0]] < 5           # the lowest index donated
        count = F.split_counts(C, "giant")
        _, after = R.split_ref(c, count)
        assert (count > 0).sum() == 1 and (after > 0).sum() > 1000 and after.sum() == 5000
        count = F.split_counts(C, "zero_one")
        out, after = R.split_ref(c, count)
        assert set(count.tolist()) == {0, 1} and np.array_equal(after, count) and np.array_equal(out, c)
        assert (F.split_counts(C, "full") > 0).all()
        count = F.split_counts(C, "random")
        assert 0 < (count == 0).sum() < C // 5 and count.max() <= 49


@pytest.mark.parametrize("C,d,per,ndup", F.TRAIN_CASES)
def test_train_inputs_with_splits_are_fair(C, d, per, ndup):
    """per iteration: the smallest gap between a point's nearest centroid and the nearest different row exceeds the chain's
    rounding bound for two distances (so no exact tie between different rows either), and the float32 and float64 numpy
    Lloyd agree.  The first iteration, and only it, splits."""
    x, rows = F.train_case(C, d, per, ndup)
    assert np.linalg.norm(x.astype(np.float64), axis=1).max() < 1.2
    ref64, trace64 = F.lloyd_trace(x, x[rows], F.TRAIN_NITER, np.float64)
    ref32, trace32 = F.lloyd_trace(x, x[rows], F.TRAIN_NITER, np.float32)
    plain = R.lloyd_ref(x, x[rows], F.TRAIN_NITER)
    for got, want in zip(ref64, plain):
        assert np.array_equal(got, want)         # the trace is lloyd_ref
    print(f"train ({C},{d},{per},{ndup}): empties {[t['empties'] for t in trace64]} changed {[t['changed'] for t in trace64]}")
    print("  gaps " + " ".join(f"{t['gap']:.3e}" for t in trace64) + f"  bound {F.train_bound(d):.3e}")
    assert [t["empties"] for t in trace64[:-1]] == [ndup] + [0] * (F.TRAIN_NITER - 1)
    assert trace64[0]["changed"] == len(x) and trace64[1]["changed"] > 0 and all(t["changed"] == 0 for t in trace64[2:])
    for t64, t32 in zip(trace64, trace32):
        assert t64["gap"] > F.train_bound(d) and t32["gap"] > 0.0
        assert (t64["empties"], t64["changed"]) == (t32["empties"], t32["changed"])
    assert np.linalg.norm(ref64[0].astype(np.float64), axis=1).max() < 1.2
    assert np.array_equal(ref64[3], ref32[3]) and np.array_equal(ref64[2], ref32[2]) and np.array_equal(ref64[0], ref32[0])
    assert (ref64[2] > 0).all() and ref64[2].sum() == len(x)


def test_nonfinite_case_has_the_rows_it_claims():
    for centroid_nan in (False, True):
        x, c = F.nonfinite_case(centroid_nan)
        assert x.shape == (130, 8) and c.shape == (5, 8)
        assert np.isnan(x[0]).sum() == 1 and np.isposinf(x[1]).sum() == 1 and not x[2].any() and np.isfinite(x[3:]).all()
        assert np.isnan(c).sum() == int(centroid_nan) and c[0, 2] < 0 < c[1, 2]


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_fit_refuses_nonfinite_input_before_any_launch(stubbed, bad):
    kmeans, calls = stubbed
    x = np.random.RandomState(0).randn(64, 8).astype(np.float32)
    x[17, 3] = bad
    with pytest.raises(ValueError, match="finite"):
        kmeans.KMeans(n_clusters=4, n_init=2, max_iter=3, device="cpu").fit(x)
    with pytest.raises(ValueError, match="finite"):
        kmeans.KMeans(n_clusters=4, n_init=2, max_iter=3, device="cpu").fit(torch.from_numpy(x))
    assert calls == []
    x[17, 3] = 0.0
    assert kmeans.KMeans(n_clusters=4, n_init=2, max_iter=3, device="cpu").fit(x).n_train_ == 64 and len(calls) == 2
