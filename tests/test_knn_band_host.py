"""CPU: the worst-case-rounding inputs of tests/bandfx.py do what tests/test_gpu_knn_band.py needs them to do, judged by the CPU
oracle's knn alone -- for every (metric, d, k, layout, n) the GPU file uses:

* rho <= 1 for every query: the victims' filter scores are inside the band below the k-th filter score.  This is the proof of
  knn_bf16.hip's header on its worst case; if it fails the model or the bound is wrong and nothing should go to a GPU;
* at least half of the queries reach the floor of their d (bandfx.FLOORS: above 0.5 everywhere, so a band half as wide loses
  oracle rows);
* the oracle's top-k and the filter's own top-k (by s~) differ in at least k/2 rows for every query: the case contests something;

and to_fp16 is what k_convert_bf16 stores: numpy's float16 cast on normal values, saturation and flush at the edges."""
import numpy as np
import pytest

from tests import bandfx as fx


def test_the_floors_leave_no_room_for_a_halved_band():
    assert set(fx.FLOORS) == set(fx.DIMS) == set(fx.LOWERED)
    for d, (floor, reached) in fx.FLOORS.items():
        assert 0.5 < floor <= reached - 0.03 + 1e-9, d
    assert {k for _, _, k, _, _ in fx.data_cases()} == {1, 10, 64}
    reach = {}
    for kernel, _, _, metric, _, layout, k, _ in fx.rounding_cases():
        reach.setdefault(kernel, set()).add((metric, layout))
        reach.setdefault(kernel + "/k", set()).add(k)
    for kernel in ("scan_bf16", "qs", "qs2", "qs4", "qsw"):
        assert reach[kernel] == {(m, lay) for m in ("ip", "l2") for lay in fx.LAYOUTS} and reach[kernel + "/k"] == {1, 10, 64}


@pytest.mark.parametrize("metric,d,k,layout,n", fx.data_cases())
def test_the_victims_sit_deep_in_the_band_and_never_outside(oracle, metric, d, k, layout, n):
    X, Q = fx.case_data(metric, d, k, layout, n)
    assert X.shape == (n, d) and Q.shape == (fx.N_QUERIES, d) and n % 64 != 0
    _, I = oracle.knn(metric, X, Q, k)
    S, eps = fx.filter_scores(metric, X, Q)
    rho = fx.tightness(metric, X, Q, k, I, (S, eps))
    floor = fx.FLOORS[d][0]
    print(f"rho: max {rho.max():.4f} median {np.median(rho):.4f} min {rho.min():.4f} (floor {floor})")
    assert rho.max() <= 1.0, "a row of the exact top-k lies outside the band: the bound or its model is wrong"
    assert (rho >= floor).sum() * 2 >= len(rho)
    top = fx.filter_topk(S, k)
    shared = np.array([len(np.intersect1d(I[q], top[q])) for q in range(len(Q))])
    assert (k - shared >= k / 2).all()
    # both query families are there: fp16-exact queries and queries with a rounding residual
    qres = ((Q.astype(np.float64) - fx.to_fp16(Q).astype(np.float64)) ** 2).sum(1)
    assert (qres == 0).sum() >= len(Q) // 2 and (qres > 0).sum() >= len(Q) // 4
    # the fillers: at least 3 x REFRESH rows below the band of every query in the filter score
    lo = np.partition(-S, k - 1, axis=1)[:, k - 1] * -1.0 - 2.0 * eps
    assert ((S < lo[:, None]).sum(1) >= fx.N_FILLER_MIN).all()
    # ... and inside it, besides both top-k, rows that are in neither -- with the impostors more than REFRESH appends behind the
    # victims, and no more in all than the smallest list holds without settling the band exactly
    in_band = (S > lo[:, None]).sum(1)
    assert (in_band >= 2 * k + 8 + fx.n_neutral(k)).all() and (in_band <= 192).all()
    assert fx.n_neutral(k) + k + 8 > fx.REFRESH


def test_to_fp16_is_the_float16_cast_on_normal_values():
    rng = np.random.default_rng(1)
    v = (rng.standard_normal(200000) * np.exp(rng.uniform(np.log(2.0 ** -14), np.log(65504.0), 200000))).astype(np.float32)
    v = v[(np.abs(v) >= 2.0 ** -14) & (np.abs(v) <= 65504.0)]
    assert len(v) > 100000
    assert np.array_equal(fx.to_fp16(v).view(np.uint16), v.astype(np.float16).view(np.uint16))


@pytest.mark.parametrize("v,want", [
    (65504.0, 65504.0), (65519.99, 65504.0), (65520.0, 65504.0), (1e6, 65504.0), (3e19, 65504.0),      # saturation, not inf
    (2.0 ** -14, 2.0 ** -14), (np.nextafter(np.float32(2.0 ** -14), np.float32(0)), 2.0 ** -14),       # rounds UP to the least normal
    (2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -14),                                                         # the tie goes to even: 2^-14
    (2.0 ** -14 * (1 - 2.0 ** -10), 0.0), (2.0 ** -15, 0.0), (2.0 ** -24, 0.0), (1e-30, 0.0), (0.0, 0.0),   # subnormal results flush
    (1.0, 1.0), (1.0 + 2.0 ** -11, 1.0), (1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -9),                       # ties to even
])
def test_to_fp16_at_the_saturation_and_flush_boundaries(v, want):
    for sign in (1.0, -1.0):
        got = fx.to_fp16(np.array([sign * v], dtype=np.float32))
        assert got.dtype == np.float16 and float(got[0]) == sign * want
        assert np.signbit(got[0]) == (sign < 0) or want == 0.0


def test_band_eps_is_band_eps_raw():
    # hand-computed from the formula in knn_bf16.hip's header, in float64: the float32 transcription agrees to float32 precision
    d, qn, qres2, xn2, xr2, xh2 = 768, 1.21, 3e-8, 4.0, 2.5e-7, 3.9
    nq = np.sqrt(qn) * 1.0005
    ip = (nq * np.sqrt(xr2) + np.sqrt(qres2) * np.sqrt(xh2)) * 1.002 + 3.0 * d * 2.0 ** -24 * nq * np.sqrt(xn2) * 1.002
    assert fx.band_eps(d, qn, qres2, xn2, xr2, xh2, False) == pytest.approx(ip, rel=1e-6)
    assert fx.band_eps(d, qn, qres2, xn2, xr2, xh2, True) == pytest.approx(2.0 * ip + 4.8e-7 * (qn + xn2), rel=1e-6)
    # an all-zero query against an overflowed residual maximum: 0 * inf admits everything
    assert fx.band_eps(d, 0.0, 0.0, np.inf, np.inf, 4e9, False) == np.inf
    assert fx.band_eps(d, [0.0, 1.0], [0.0, 0.0], 1.0, 0.0, 1.0, False)[0] == np.float32(1e-30)
