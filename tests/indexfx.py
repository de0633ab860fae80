"""Shared by tests/test_index_state_host.py (CPU) and tests/test_gpu_index_state.py (GPU): the shape tables of the index-state
tests, the host-side view of what those shapes make the scans do, the data, and the one checked call.

The principle of the GPU tests: every checked call on a REUSED handle is immediately preceded, on that handle, by a dirtying
call whose results outrank every true result of the checked call, and is compared bit for bit with the same call on a FRESH
handle and with the CPU oracle.  Whatever a workspace keeps from the dirtying call would win the merge and show.

  IP   the data lie in a cone (every inner product of two rows is well above zero); the dirtying queries are the checked
       queries times 4, so that their 64th best inner product exceeds the checked call's best;
  L2   the first L2_BLOB database rows are a tight blob; the dirtying queries are blob rows themselves (distance 0 to
       themselves, ~1e-3 to the 64th nearest), the checked queries are no database rows and lie ~1 away from everything.
Nothing here is assumed by the tests: they assert the outranking from the results of the two calls."""
import ctypes

import numpy as np

F32, BF16 = 1, 2
MAX_K = 64              # LEMON_MAX_K: the k of every dirtying call
ROWS = 128              # database tile = query panel of the fp32 scan; index capacity is rounded to it
ORACLE_SAMPLE = 300     # queries of a checked call that are also compared with the CPU oracle

# ---- fp32 scan: one handle, this sequence of (nq, k) --------------------------------------------------------------------------
F32_D, F32_N = 40, 128 * 37
# (65400 queries are 511 panels: the one plan here in which every panel is scanned in one piece, so that no merge runs)
F32_SEQUENCE = [(700, 20), (130, 64), (1, 1), (66000, 10), (5, 51), (257, 33), (900, 5), (65400, 7), (0, 3), (700, 20)]

# ---- 16-bit scan: per handle ("add", rows) and ("search", knob, nq, k) steps; knob as in tests/golden/knn_bf16_plan.txt -------
BF16_HANDLES = [
    dict(d=768, wide=False, steps=[
        ("add", 1900),
        ("search", "CHUNK_MB=0.01", 300, 20),         # launches of 8 and 7 tiles, state carried between them
        ("search", "CHUNK_MB=0.01", 130, 7),          # the same with fewer queries and a smaller k
        ("search", "defaults", 300, 10),              # one launch over the same ws_state / ws_cand
        ("search", "QS2_MIN_PANELS=0", 300, 33),      # 256-query panels (qs4 / qs2)
        ("add", 1100),
        ("search", "CHUNK_MB=0.01", 300, 20),         # 3 database splits and a merge
        ("search", "CHUNK_MB=0.01", 130, 7),
    ]),
    dict(d=1000, wide=False, steps=[                  # the streaming kernel (768 < d, wide filter off)
        ("add", 3000),
        ("search", "defaults", 150, 20),
        ("search", "defaults", 70, 5),
        ("search", "defaults", 150, 12),
    ]),
    dict(d=1000, wide=False, steps=[                  # the wide filter switched on and off again: the 16-bit copy changes its pitch
        ("add", 3000),
        ("search", "defaults", 150, 20),
        ("wide", True),
        ("search", "QS2_MIN_PANELS=0", 150, 20),      # qsw at pitch 1024
        ("wide", False),
        ("search", "defaults", 150, 5),
    ]),
]

# ---- fp32 scan: a call of more than one query chunk (QCHUNK = 2^19 queries in knn_f32.hip), then a small one ------------------
CHUNKED_D, CHUNKED_N = 24, 2000
CHUNKED_SEQUENCE = [((1 << 19) + 130, 3), (700, 20)]

# ---- switching algorithms on one handle: (algo, nq, k) at d = 768 -------------------------------------------------------------
SWITCH_D, SWITCH_N = 768, 1900
SWITCH_SEQUENCE = [(F32, 600, 20), (BF16, 130, 33), (F32, 257, 5), (BF16, 900, 20), (F32, 70, 64), (BF16, 300, 1)]


def scan_plan(panels, n_tiles):
    """lemon_debug_scan_plan (host only, no device is touched): the fp32 scan's grid, splits and pieces per panel"""
    from lemon_amd import _lib
    lib = _lib.load()
    cap_wgs, cap_segs = 4096, panels * 8 + 8192
    g, sp, ns = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    sb = np.zeros(cap_wgs + 1, np.int32)
    pc = np.zeros(panels, np.int32)
    sg = np.zeros(4 * cap_segs, np.int32)
    ip = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_int))
    rc = lib.lemon_debug_scan_plan(panels, n_tiles, ctypes.byref(g), ctypes.byref(sp), ip(sb), cap_wgs, ip(pc), ip(sg), cap_segs,
                                   ctypes.byref(ns))
    assert rc == 0
    # seg_begin [grid + 1]: first segment of every workgroup; segs [n_segs, 4]: (panel, first tile, tiles, piece in the panel)
    return dict(grid=g.value, splits=sp.value, pieces=pc.copy(), seg_begin=sb[:g.value + 1].copy(),
                segs=sg[:4 * ns.value].reshape(-1, 4).copy())


def f32_steps(sequence=F32_SEQUENCE, n=F32_N):
    """one dict per NON-EMPTY call of the fp32 sequence: the plan key (panels, n_tiles), nq_pad, kk, splits, pieces.  A pair of
    fewer than 2 units has no plan (lemon_search_f32_pass): one workgroup, no merge."""
    n_tiles = (n + ROWS - 1) // ROWS
    out = []
    for nq, k in sequence:
        if nq == 0:
            continue
        panels = (nq + ROWS - 1) // ROWS
        if panels * n_tiles >= 2:
            pl = scan_plan(panels, n_tiles)
        else:
            pl = dict(grid=1, splits=1, pieces=np.ones(1, np.int32))
        out.append(dict(nq=nq, kk=k, panels=panels, n_tiles=n_tiles, nq_pad=panels * ROWS, **pl))
    return out


def bf16_steps(handle, l2):
    """the recorded plan rows (tests/golden/knn_bf16_plan.txt) of a 16-bit handle's searches, with the knob, nq, k and n of each"""
    from tests.test_knn_bf16_plan_host import planned
    n, wide, out = 0, handle["wide"], []
    for step in handle["steps"]:
        if step[0] == "add":
            n += step[1]
            continue
        if step[0] == "wide":
            wide = step[1]
            continue
        _, knob, nq, k = step
        rows = planned(knob, handle["d"], wide, l2, n, nq)
        assert len(rows) == 1, "the sequences use one query chunk per call"
        out.append(dict(knob=knob, nq=nq, k=k, n=n, wide=wide, **rows[0]))
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------------
L2_BLOB = 80            # leading database rows of an L2 index that form the tight blob the dirtying queries come from
_CONE, _BLOB_SPREAD = 0.8, 0.02


def is_l2(metric):
    return metric in ("l2", "euclidean")


def _gauss(rng, n, d):
    return rng.standard_normal((n, d)) / np.sqrt(d)           # rows of norm ~1


def _f32c(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def cone_axis(d):
    return np.where(np.arange(d) % 3 == 0, -1.0, 1.0) / np.sqrt(d)


def cone_rows(rng, n, d, spread=_CONE):
    """unit rows around one fixed direction: <a, b> ~ 1 / (1 + spread^2) for any two of them (0.6 by default)"""
    x = cone_axis(d)[None, :] + spread * _gauss(rng, n, d)
    return _f32c(x / np.linalg.norm(x, axis=1, keepdims=True))


def make_db(rng, n, d, metric):
    """n database rows, not unit: IP a cone, L2 a tight blob of min(n, L2_BLOB) rows followed by spread-out rows"""
    scale = rng.uniform(0.8, 1.25, (n, 1))
    if not is_l2(metric):
        return _f32c(cone_rows(rng, n, d) * scale)
    x = _gauss(rng, n, d)
    x = x / np.linalg.norm(x, axis=1, keepdims=True) * scale
    nb = min(n, L2_BLOB)
    x[:nb] = x[0][None, :] + _BLOB_SPREAD * _gauss(rng, nb, d)
    return _f32c(x)


def make_queries(rng, nq, d, metric):
    """nq checked queries: no database rows"""
    if not is_l2(metric):
        return cone_rows(rng, nq, d)
    x = _gauss(rng, nq, d)
    return _f32c(x / np.linalg.norm(x, axis=1, keepdims=True))


def dirty_queries(X, Q, metric):
    """the dirtying queries of a checked call with queries Q on a database that starts with X's rows: as many as Q has, and for
    L2 with Q's pattern of repeated rows wherever that can be kept (row i is blob row i mod blob size)"""
    if not is_l2(metric):
        return _f32c(Q * np.float32(4.0))
    nb = min(X.shape[0], L2_BLOB)
    return _f32c(X[np.arange(Q.shape[0]) % nb])


def more_rows(rng, m, d, metric):
    """m further database rows of make_db's kind (for L2 without a second blob)"""
    return make_db(rng, m + L2_BLOB, d, metric)[L2_BLOB:]


# ---- the add life cycle: 1900 rows, 20 more within the capacity of 1920, 1 more (capacity grows), 1100 more -------------------
ADD_D, ADD_NQ, ADD_K = 192, 200, 10
ADD_STEPS = (1900, 20, 1, 1100)
ADD_BIG_STEPS = (1, 2)              # the steps whose rows have four times the norm of the others
ADD_MIN_HITS = 32                   # queries of every later call that must have one of those rows among their k best


def big_rows(rng, m, d, metric):
    """m rows of norm 4.  IP: well off the cone's axis (cosine ~0.3 to a query), so that 4 x 0.3 puts them among the best of most
    queries and yet below 4 x the 64th best ordinary row, which is what the dirtying call needs.  L2: anywhere."""
    if is_l2(metric):
        x = _gauss(rng, m, d)
    else:
        x = 0.42 * cone_axis(d)[None, :] + _gauss(rng, m, d)
    return _f32c(4.0 * x / np.linalg.norm(x, axis=1, keepdims=True))


def add_cycle(rng, metric, d=ADD_D, nq=ADD_NQ):
    """[(rows added, queries of the search behind the add)] of the add life cycle.  L2: once big rows exist the first 40 queries
    lie 0.9 away from one of them (and >= 2.7 from every other row), so that it is their nearest neighbour."""
    out, big = [], np.zeros((0, d), np.float32)
    for i, m in enumerate(ADD_STEPS):
        if i == 0:
            rows = make_db(rng, m, d, metric)
        elif i in ADD_BIG_STEPS:
            rows = big_rows(rng, m, d, metric)
            big = np.concatenate([big, rows])
        else:
            rows = more_rows(rng, m, d, metric)
        Q = make_queries(rng, nq, d, metric)
        if is_l2(metric) and len(big):
            Q[:40] = big[np.arange(40) % len(big)] + 0.9 * _gauss(rng, 40, d)
        out.append((rows, _f32c(Q)))
    return out


# ---- LemonDB across splits ----------------------------------------------------------------------------------------------------
DB_N, DB_SMALL_N, DB_CLASSES = 300, 20, 12
DB_TRAIN_NQ, DB_VAL_NQ, DB_K = 1200, 200, 50
_DB_CONE = 0.5          # a narrower cone: 4 x the WORST of DB_SMALL_N rows still has to beat the best of them


def lemon_db_data(rng, ndb, d, metric):
    """image / text database rows (the text rows are class prompts: few distinct ones, behind the blob for L2) with their class
    numbers, and a maker of query splits.  IP rows are unit rows, as the product's are."""
    l2 = is_l2(metric)
    img = make_db(rng, ndb, d, metric) if l2 else cone_rows(rng, ndb, d, _DB_CONE)
    protos = make_queries(rng, DB_CLASSES, d, metric)
    lab = rng.integers(0, DB_CLASSES, ndb).astype(np.int32)
    txt = make_db(rng, ndb, d, metric) if l2 else protos[lab].copy()
    first = min(ndb, L2_BLOB) if l2 else 0            # (L2: the blob rows keep their own text rows)
    txt[first:] = protos[lab[first:]]

    def split(nq, train):
        """nq queries; train: two of three are database rows (in_db = 1; L2: never blob rows), the others are not -- none is where
        the database is smaller than L2_BLOB (its worst row is then no match for a query's own row, whatever the dirtying)"""
        q_img = make_queries(rng, nq, d, metric) if l2 else cone_rows(rng, nq, d, _DB_CONE)
        q_lab = rng.integers(0, DB_CLASSES, nq).astype(np.int32)
        in_db = np.zeros(nq, np.uint8)
        if train and ndb > L2_BLOB:
            rows = first + np.arange(nq) % (ndb - first)
            in_db = (np.arange(nq) % 3 != 0).astype(np.uint8)
            q_img[in_db == 1] = img[rows[in_db == 1]]
            q_lab[in_db == 1] = lab[rows[in_db == 1]]
        return dict(q_img=_f32c(q_img), q_txt=_f32c(protos[q_lab]), q_lab=q_lab, in_db=in_db)

    return dict(img=_f32c(img), txt=_f32c(txt), lab=lab, split=split)


def lemon_db_case(d, metric):
    """the data of one LemonDB test case: the database of DB_N rows with its train and val splits, and the database of
    DB_SMALL_N rows (fewer than DB_K: padded records) with a val split and a train-style split of rows that are not in it"""
    rng = np.random.default_rng(61 + d)
    data = lemon_db_data(rng, DB_N, d, metric)
    data["train"], data["val"] = data["split"](DB_TRAIN_NQ, True), data["split"](DB_VAL_NQ, False)
    small = lemon_db_data(rng, DB_SMALL_N, d, metric)
    small["val"], small["train"] = small["split"](DB_VAL_NQ, False), small["split"](DB_TRAIN_NQ, True)
    return data, small


def repeated(rng, protos, nq):
    """nq rows drawn from `protos`, every prototype at least once"""
    C = protos.shape[0]
    assign = rng.integers(0, C, nq)
    assign[:C] = np.arange(C)
    return _f32c(protos[assign])


def n_distinct(Q):
    return len({r.tobytes() for r in Q})


def sample_rows(nq):
    """at most ORACLE_SAMPLE query numbers, spread over the whole call (first and last included)"""
    return np.unique(np.linspace(0, nq - 1, min(nq, ORACLE_SAMPLE)).astype(np.int64)) if nq else np.zeros(0, np.int64)


# ---- the checked call ---------------------------------------------------------------------------------------------------------
def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def new_index(hip, metric, d, algo, X=None, dedup=None, wide=False):
    """a fresh handle with the settings a reused one was given"""
    ix = (hip.IndexFlatL2 if is_l2(metric) else hip.IndexFlatIP)(d)
    ix.set_algo(algo)
    if dedup is not None:
        ix.set_query_dedup(dedup)
    if wide:
        ix.set_wide_filter(True)
    if X is not None and len(X):
        ix.add(cu(X))
    return ix


def bits_equal(a, b):
    """bit-for-bit equality of two tensors (float32 through int32, so that -0.0 / NaN payloads count)"""
    import torch
    if a.dtype == torch.float32:
        a, b = a.view(torch.int32), b.view(torch.int32)
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a, b))


def assert_outranked(D_dirty, D_checked, metric, n_db):
    """the dirtying precondition, from the results: for EVERY query the dirtying call's last existing key (column
    min(k, n_db) - 1) is strictly better than the checked call's best key"""
    last = D_dirty[:, min(D_dirty.shape[1], n_db) - 1]
    best = D_checked[:, 0]
    assert last.shape == best.shape and last.numel() > 0
    ok = (last < best) if is_l2(metric) else (last > best)
    assert bool(ok.all()), f"{int((~ok).sum())} queries whose dirtying results do not outrank the checked call's best"


def assert_equals_oracle(oracle, metric, X, Q, k, D, I):
    """(D, I) tensors of search(Q, k) over the rows X against the CPU oracle, bit for bit, on sample_rows of the queries"""
    rows = sample_rows(Q.shape[0])
    Do, Io = oracle.knn("euclidean" if is_l2(metric) else "cosine", X, Q[rows], k)
    rt = cu(rows)
    assert np.array_equal(I[rt].cpu().numpy(), Io), "I differs from the oracle's"
    assert np.array_equal(D[rt].cpu().numpy().view(np.int32), Do.view(np.int32)), "D differs from the oracle's"


def checked_search(reused, fresh, X, Q, k, metric, oracle, after_dirty=None):
    """dirty `reused` (same nq, k = MAX_K), run search(Q, k) on it, and hold the result against `fresh` (a handle with the same
    settings and rows that has served nothing) and against the oracle on a sample.  X: the rows of both handles.  after_dirty:
    called with the reused handle between the two calls (for assertions on what the dirtying call did).  -> (D, I) tensors"""
    qd, qt = cu(dirty_queries(X, Q, metric)), cu(Q)
    Dd, _ = reused.search(qd, MAX_K)
    if after_dirty is not None:
        after_dirty(reused)
    D, I = reused.search(qt, k)
    assert_outranked(Dd, D, metric, X.shape[0])
    Df, If = fresh.search(qt, k)
    assert bits_equal(I, If), f"I differs from the fresh handle's in {int((I != If).sum())} places"
    assert bits_equal(D, Df), f"D differs from the fresh handle's in {int((D != Df).sum())} places"
    assert_equals_oracle(oracle, metric, X, Q, k, D, I)
    return D, I
