"""GPU: the k-means kernels (lemon_amd/csrc/kmeans.hip) at their tile, k-slice, panel, wave and key-bit edges.

assign is held to the flat index bit for bit (the header's contract) and, independently, to float64 within the chain's
rounding bound; update, objective and split run through the C ABI inside poisoned, guarded allocations against the float64
numpy rules of tests/kmeans_ref.py; the train loop is run on inputs whose first iteration splits.  The inputs come from
tests/kmeansfx.py; tests/test_kmeans_edges_host.py shows on the CPU that they are fair."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import kmeans_ref as R
from tests import kmeansfx as F

pytestmark = pytest.mark.gpu

POISON = 0xA5
GUARD = 4096


class Guarded:
    """A device array inside an allocation of its own with GUARD poisoned bytes on either side."""

    def __init__(self, arr):
        arr = np.ascontiguousarray(arr)
        self.dtype, self.shape, self.nbytes = arr.dtype, arr.shape, arr.nbytes
        host = np.full(2 * GUARD + arr.nbytes, POISON, np.uint8)
        host[GUARD:GUARD + arr.nbytes] = arr.reshape(-1).view(np.uint8)
        self.buf = torch.from_numpy(host).cuda()

    @classmethod
    def poisoned(cls, shape, dtype):
        return cls(np.full(int(np.prod(shape)) * np.dtype(dtype).itemsize, POISON, np.uint8).view(dtype).reshape(shape))

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + GUARD)

    def read(self):
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == POISON).all() and (host[GUARD + self.nbytes:] == POISON).all(), "guard overwritten"
        return host[GUARD:GUARD + self.nbytes].view(self.dtype).reshape(self.shape).copy()


def _bits(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def _flat_search(x, c):
    from lemon_amd import IndexFlatL2
    idx = IndexFlatL2(c.shape[1], c.device)
    idx.add(c)
    D, I = idx.search(x, 1)
    return I[:, 0], D[:, 0]


def _assign_poisoned(x, c):
    """kmeans.assign into poisoned out= buffers, checked against the flat search bit for bit -> (a int64, dist) on the host"""
    from lemon_amd import kmeans
    n = x.shape[0]
    xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(c).cuda()
    a = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    dist = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    kmeans.assign(xd, cd, out=(a, dist))
    I, D = _flat_search(xd, cd)
    a, dist, I, D = a.cpu().numpy().astype(np.int64), dist.cpu().numpy(), I.cpu().numpy(), D.cpu().numpy()
    assert np.array_equal(a, I), np.flatnonzero(a != I)[:8]
    assert np.array_equal(dist.view(np.int32), D.view(np.int32)), np.flatnonzero(dist.view(np.int32) != D.view(np.int32))[:8]
    return a, dist


# ---- 1. assign at tile, slice and panel edges -------------------------------------------------------------------------
@pytest.mark.parametrize("n,C,d", F.assign_shapes())
def test_assign_at_tile_slice_and_panel_edges(hip, n, C, d):
    for unit_centroids in (True, False):
        x, c = F.assign_case(n, C, d, unit_centroids)
        a, dist = _assign_poisoned(x, c)
        differ = F.check_against_float64(x, c, a, dist)
        print(f"assign ({n},{C},{d},{'unit' if unit_centroids else 'scaled'}): {differ} of {n} assignments differ from float64")
        if C >= 8:                               # the planted rows: tie -> lower index, distance exactly 0
            for j in range(min(n, 3)):
                want = {C - 1: 5, C // 2: 0}.get((j * 7) % C, (j * 7) % C)
                assert a[j] == want and dist[j] == 0.0, (j, a[j], want, dist[j])
            assert not np.isin(a, [C - 1, C // 2]).any()


# ---- 2. tie table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 36])
@pytest.mark.parametrize("pair", F.TIE_PAIRS, ids=[f"{a}_{b}" for a, b in F.TIE_PAIRS])
def test_tie_goes_to_the_lower_index_across_lanes_groups_and_tiles(hip, pair, d):
    """bitwise-duplicate rows give bit-identical keys: the lower index wins whichever lane half, 32-row group or centroid
    tile holds it, for every point (exact, not statistical)"""
    x, c, lo, hi = F.tie_case(pair, d)
    a, dist = _assign_poisoned(x, c)
    assert a[0] == lo and dist[0] == 0.0, (a[0], dist[0])
    assert not (a == hi).any(), np.flatnonzero(a == hi)
    assert (a == lo).sum() >= 50                 # the host test shows that float64 sends at least 50 points to the pair
    F.check_against_float64(x, c, a, dist)


# ---- 3. non-finite rows -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("centroid_nan", [False, True])
def test_assign_on_nonfinite_rows_equals_the_flat_search(hip, centroid_nan):
    x, c = F.nonfinite_case(centroid_nan)
    a, dist = _assign_poisoned(x, c)
    print(f"non-finite rows (centroid NaN {centroid_nan}): a[:3] = {a[:3].tolist()} dist[:3] = {dist[:3].tolist()}")
    if not centroid_nan:                         # the finite rows are untouched by their neighbours in the panel
        F.check_against_float64(x[3:], c, a[3:], dist[3:])


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), float("-inf")])
def test_fit_refuses_nonfinite_input(hip, bad, monkeypatch):
    from lemon_amd import kmeans
    x = torch.from_numpy(F.unit_rows(np.random.RandomState(1), 130, 8)).cuda()
    x[77, 5] = bad
    monkeypatch.setattr(kmeans, "train", lambda *a, **k: pytest.fail("train was launched"))
    with pytest.raises(ValueError, match="finite"):
        kmeans.KMeans(n_clusters=5, n_init=1, max_iter=2).fit(x)
    with pytest.raises(ValueError, match="finite"):
        kmeans.KMeans(n_clusters=5, n_init=1, max_iter=2).fit(x.cpu().numpy())


# ---- 4. / 5. update and objective through the C ABI ----------------------------------------------------------------------
def _update_abi(x, a, dist, c):
    """lemon_kmeans_update with the centroid matrix, count, obj and the workspace poisoned and guarded -> (c, count, obj)"""
    from lemon_amd import _lib
    from lemon_amd.ops import stream_ptr
    lib = _lib.load()
    n, d = x.shape
    C = c.shape[0]
    dev = torch.device("cuda")
    xd, ad, dd = torch.from_numpy(x).to(dev), torch.from_numpy(a).to(dev), torch.from_numpy(dist).to(dev)
    cg, ng, og = Guarded(c), Guarded.poisoned((C,), np.int64), Guarded.poisoned((1,), np.float64)
    ws_bytes = int(lib.lemon_kmeans_workspace_bytes(n, d, C))
    assert ws_bytes > 0
    wg = Guarded.poisoned((ws_bytes,), np.uint8)
    vp = ctypes.c_void_p
    _lib.check(lib.lemon_kmeans_update(vp(xd.data_ptr()), n, d, vp(ad.data_ptr()), vp(dd.data_ptr()), C, cg.ptr, ng.ptr, og.ptr,
                                       wg.ptr, ws_bytes, stream_ptr(dev)), "lemon_kmeans_update")
    torch.cuda.synchronize()
    wg.read()
    assert np.array_equal(xd.cpu().numpy().view(np.int32), x.view(np.int32)) and np.array_equal(ad.cpu().numpy(), a)     # only read
    return cg.read(), ng.read(), og.read()


def _check_obj(obj, dist, what):
    want = math.fsum(dist.astype(np.float64).tolist())
    rel = abs(float(obj[0]) - want) / max(want, 1e-300)
    print(f"{what}: obj relative error {rel:.3e}")
    assert rel <= 1e-12


@pytest.mark.parametrize("n,C,d,pattern", F.UPDATE_CASES)
def test_update_with_crafted_assignments(hip, n, C, d, pattern):
    rs = np.random.RandomState(n + C + d)
    x = rs.randn(n, d).astype(np.float32)
    c = rs.randn(C, d).astype(np.float32)
    dist = rs.rand(n).astype(np.float32)
    a = F.crafted_assign(n, C, pattern)
    got, count, obj = _update_abi(x, a, dist, c)
    got2, count2, obj2 = _update_abi(x, a, dist, c)
    assert np.array_equal(_bits(got), _bits(got2)) and np.array_equal(count, count2) and np.array_equal(_bits(obj), _bits(obj2))

    want, want_count = F.update_expected(x, a, c)
    assert np.array_equal(count, want_count)     # out-of-range points are counted nowhere
    full = want_count > 0
    assert np.array_equal(got[~full].view(np.int32), c[~full].view(np.int32))      # an empty cluster keeps its bits
    if full.any():
        err = np.abs(got[full].astype(np.float64) - want[full].astype(np.float64))
        ulp = np.spacing(np.abs(want[full])).astype(np.float64)
        print(f"update ({n},{C},{d},{pattern}): max error {float((err / ulp).max()):.3f} ulp")
        assert (err <= ulp).all()                # one ulp: another float64 order can flip the final rounding
    _check_obj(obj, dist, f"update ({n},{C},{d},{pattern})")


@pytest.mark.parametrize("n", F.OBJ_N)
def test_objective_below_at_and_above_one_block(hip, n):
    rs = np.random.RandomState(n)
    x = rs.randn(n, 4).astype(np.float32)
    dist = (rs.rand(n) * rs.choice([1e-3, 1.0, 1e3], n)).astype(np.float32)
    a, c = np.zeros(n, np.int32), np.zeros((1, 4), np.float32)
    _, count, obj = _update_abi(x, a, dist, c)
    _, _, obj2 = _update_abi(x, a, dist, c)
    assert count.tolist() == [n] and np.array_equal(_bits(obj), _bits(obj2))
    _check_obj(obj, dist, f"objective n = {n}")


# ---- 6. split at reduction edges ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,d,pattern", F.split_cases())
def test_split_at_reduction_edges(hip, C, d, pattern):
    from lemon_amd import _lib
    from lemon_amd.ops import stream_ptr
    c, count = F.split_case(C, d, pattern)
    want_c, want_count = R.split_ref(c, count)
    cg, ng = Guarded(c), Guarded(count)
    _lib.check(_lib.load().lemon_kmeans_split(cg.ptr, d, C, ng.ptr, stream_ptr(torch.device("cuda"))), "lemon_kmeans_split")
    torch.cuda.synchronize()
    got_c, got_count = cg.read(), ng.read()
    assert np.array_equal(got_count, want_count), np.flatnonzero(got_count != want_count)[:8]
    assert np.array_equal(got_c.view(np.int32), want_c.view(np.int32)), np.flatnonzero((got_c.view(np.int32) != want_c.view(np.int32)).any(1))[:8]
    if pattern in ("zero_one", "full"):
        assert np.array_equal(got_c.view(np.int32), c.view(np.int32)) and np.array_equal(got_count, count)


# ---- 7. train with splits inside the loop -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def train_refs():
    out = {}
    for case in F.TRAIN_CASES:
        x, rows = F.train_case(*case)
        out[case] = (x, rows) + F.lloyd_trace(x, x[rows], F.TRAIN_NITER)
    return out


@pytest.mark.parametrize("case", F.TRAIN_CASES, ids=["-".join(map(str, c)) for c in F.TRAIN_CASES])
def test_train_with_splits_inside_the_loop(hip, train_refs, case, monkeypatch):
    """the first iteration leaves the higher index of every duplicated start row empty and splits; tests/test_kmeans_edges_host.py
    ::test_train_inputs_with_splits_are_fair is what entitles this test to demand the float64 Lloyd's assignment exactly"""
    from lemon_amd import kmeans
    x, rows, (want_c, want_obj, want_count, want_a), trace = train_refs[case]
    assert trace[0]["empties"] == case[3]
    xd = torch.from_numpy(x).cuda()
    init = xd[torch.from_numpy(rows).cuda()]
    monkeypatch.delenv("LEMON_KMEANS_EARLY_STOP", raising=False)
    fast = [t.cpu().numpy() for t in kmeans.train(xd, init, F.TRAIN_NITER)]
    monkeypatch.setenv("LEMON_KMEANS_EARLY_STOP", "0")
    full = [t.cpu().numpy() for t in kmeans.train(xd, init, F.TRAIN_NITER)]
    for u, v in zip(fast, full):
        assert u.dtype == v.dtype and np.array_equal(_bits(u), _bits(v))
    c, obj, count, a = fast
    assert np.array_equal(a.astype(np.int64), want_a)
    assert np.array_equal(count, want_count)
    cerr = float(np.abs(c.astype(np.float64) - want_c.astype(np.float64)).max())
    oerr = float(np.abs(obj - want_obj).max())
    print(f"train {case}: max centroid difference {cerr:.3e}, max obj difference {oerr:.3e}")
    assert cerr <= 1e-6
    assert oerr <= len(x) * (x.shape[1] + 3) * 2.0 ** -24 * 2.4 ** 2
    fixed = next(i for i, t in enumerate(trace) if t["changed"] == 0 and t["empties"] == 0)
    assert 0 < fixed < F.TRAIN_NITER - 1 and (obj[fixed:] == obj[fixed]).all(), (fixed, obj)

