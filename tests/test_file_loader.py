"""CPU: the decode worker pool of file-backed datasets (lemon_amd/loader.py) and the ragged-batch plans
(lemon_amd/data.py::ragged_plan) that lemon_preprocess_ragged consumes."""
import glob
import os
import time

import numpy as np
import pytest
from PIL import Image


def _shm_segments():
    return set(glob.glob("/dev/shm/lemon_decode_*"))


def _alive(pid):
    try:
        os.kill(pid, 0)
    except ProcessLookupError:
        return False
    try:                                   # a zombie (exited, not yet reaped by someone else) does not count
        with open(f"/proc/{pid}/stat") as f:
            return f.read().split(")")[-1].split()[0] != "Z"
    except FileNotFoundError:
        return False


def _write_images(d, n=23):
    """n files of mixed formats and sizes: JPEG 4:2:0 / 4:4:4, grayscale and CMYK JPEG, palette and RGBA PNG."""
    rng = np.random.default_rng(0)
    paths = []
    for i in range(n):
        h, w = [(37, 91), (64, 48), (120, 160), (33, 33), (200, 150), (17, 250)][i % 6]
        px = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        kind = i % 6
        if kind == 0:
            p = os.path.join(d, f"{i}.jpg"); Image.fromarray(px).save(p, quality=90, subsampling=2)
        elif kind == 1:
            p = os.path.join(d, f"{i}.jpg"); Image.fromarray(px).save(p, quality=95, subsampling=0)
        elif kind == 2:
            p = os.path.join(d, f"{i}.jpg"); Image.fromarray(px[:, :, 0]).save(p, quality=90)
        elif kind == 3:
            p = os.path.join(d, f"{i}.jpg"); Image.fromarray(px).convert("CMYK").save(p, quality=90)
        elif kind == 4:
            p = os.path.join(d, f"{i}.png"); Image.fromarray(px).convert("P", palette=Image.ADAPTIVE, colors=32).save(p)
        else:
            a = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
            p = os.path.join(d, f"{i}.png"); Image.fromarray(np.concatenate([px, a], 2), "RGBA").save(p)
        paths.append(p)
    return paths


def test_pool_decodes_exactly_like_pil_in_dataset_order(tmp_path):
    from lemon_amd.loader import DecodePool
    paths = _write_images(str(tmp_path))
    before = _shm_segments()
    with DecodePool(paths, workers=3) as pool:
        assert not any(pool.torch_in_worker), "a decode worker imported torch"
        got = [(i, a.copy()) for i, a in pool.images(2, len(paths))]
        pids = list(pool.worker_pids)
    assert [i for i, _ in got] == list(range(2, len(paths)))
    for i, a in got:
        ref = np.asarray(Image.open(paths[i]).convert("RGB"))
        assert a.dtype == np.uint8 and a.shape == ref.shape and np.array_equal(a, ref), paths[i]
    assert not any(_alive(p) for p in pids)
    assert _shm_segments() == before


def test_pool_ring_stays_within_its_byte_bound(tmp_path):
    from lemon_amd.loader import DecodePool
    rng = np.random.default_rng(1)
    paths = []
    for i in range(40):
        p = os.path.join(str(tmp_path), f"{i}.png")
        Image.fromarray(rng.integers(0, 256, (300, 400, 3), dtype=np.uint8)).save(p)      # 360 KB decoded
        paths.append(p)
    ring = 2 << 20                                                                        # 2 workers x 1 MB: ~2 images each
    with DecodePool(paths, workers=2, ring_bytes=ring) as pool:
        n = 0
        for i, a in pool.images():
            assert pool.held <= pool.ring_bytes
            assert np.array_equal(a, np.asarray(Image.open(paths[i]).convert("RGB")))
            time.sleep(0.002)              # a slow consumer: the workers fill their rings and wait
            n += 1
        assert n == 40 and 0 < pool.peak_held <= pool.ring_bytes == ring


def test_pool_image_larger_than_a_ring(tmp_path):
    from lemon_amd.loader import DecodePool
    rng = np.random.default_rng(2)
    paths = []
    for i, (h, w) in enumerate([(40, 50), (700, 600), (30, 20)]):                           # 1.26 MB > a 1 MB ring
        p = os.path.join(str(tmp_path), f"{i}.png")
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(p)
        paths.append(p)
    before = _shm_segments()
    with DecodePool(paths, workers=1, ring_bytes=1 << 20) as pool:
        for i, a in pool.images():
            assert np.array_equal(a, np.asarray(Image.open(paths[i]).convert("RGB")))
    assert _shm_segments() == before


def test_corrupt_file_raises_promptly_naming_the_path(tmp_path):
    from lemon_amd.loader import DecodeError, DecodePool
    paths = _write_images(str(tmp_path), 8)
    bad = os.path.join(str(tmp_path), "broken.jpg")
    with open(bad, "wb") as f:
        f.write(b"\xff\xd8\xff\xe0 not really a jpeg" * 10)
    paths.insert(5, bad)
    paths.append(os.path.join(str(tmp_path), "missing.png"))
    before = _shm_segments()
    t0 = time.time()
    with DecodePool(paths, workers=2) as pool:
        pids = list(pool.worker_pids)
        with pytest.raises(DecodeError, match="broken.jpg"):
            for _ in pool.images():
                pass
    assert time.time() - t0 < 10
    assert not any(_alive(p) for p in pids) and _shm_segments() == before
    with DecodePool(paths, workers=2) as pool:
        with pytest.raises(DecodeError, match="missing.png"):
            for _ in pool.images(6):
                pass


def test_pool_shuts_down_on_exhaustion_early_close_and_exception(tmp_path):
    from lemon_amd.loader import DecodePool
    paths = _write_images(str(tmp_path), 30)
    before = _shm_segments()
    for how in ("exhaust", "early", "raise"):
        pool = DecodePool(paths, workers=3)
        pids = list(pool.worker_pids)
        assert all(_alive(p) for p in pids)
        try:
            with pool:
                it = pool.images()
                for i, _ in it:
                    if how == "early" and i == 4:
                        it.close()
                        break
                    if how == "raise" and i == 7:
                        raise KeyError("consumer failed")
        except KeyError:
            assert how == "raise"
        assert not any(_alive(p) for p in pids), how
        assert _shm_segments() == before, how


def test_default_worker_count_follows_usable_cpus(monkeypatch):
    from lemon_amd import loader
    monkeypatch.delenv("LEMON_DECODE_WORKERS", raising=False)
    monkeypatch.setenv("OMP_NUM_THREADS", "6")
    assert loader.usable_cpus() == min(6, len(os.sched_getaffinity(0)))
    assert loader.default_workers(1) == min(8, loader.usable_cpus())
    assert loader.default_workers(64) == 1
    monkeypatch.setenv("LEMON_DECODE_WORKERS", "0")
    assert loader.default_workers(1) == 0
    monkeypatch.setenv("LEMON_DECODE_WORKERS", "3")
    assert loader.default_workers(1) == 3


@pytest.mark.parametrize("h,w", [(2, 300), (300, 2), (100, 3000), (3000, 100), (8000, 6000), (6000, 8000), (224, 224),
                                 (32, 32), (225, 224)])
def test_ragged_plan_for_extreme_shapes(h, w):
    from lemon_amd.data import (RAGGED_HROWS, RAGGED_PLAN_INTS, pil_bicubic_rows, pil_bicubic_tables, ragged_plan,
                                resize_geometry)
    S = 224
    hdr, taps = ragged_plan(h, w, S)
    assert hdr.shape == (RAGGED_PLAN_INTS,) and hdr.dtype == np.int32 and taps.dtype == np.int32
    H, W, o_kkh, o_bh, o_kkv, o_bv, ks_h, ks_v, R, nvblk, vmin, rows, nhblk = (int(v) for v in hdr[:13])
    assert (H, W) == (h, w) and R >= 1 and R * (2 + ks_v) <= 4096 and nvblk == -(-S // R)
    assert nhblk == -(-rows // RAGGED_HROWS)
    kk_h = taps[o_kkh:o_bh].reshape(S, ks_h); b_h = taps[o_bh:o_kkv].reshape(S, 2)
    kk_v = taps[o_kkv:o_bv].reshape(S, ks_v); b_v = taps[o_bv:].reshape(S, 2)
    nh, nw, top, left = resize_geometry(h, w, S)
    # the S kept rows / columns equal the crop of the full table (built in full only where that is cheap)
    for kk, b, n_in, n_out, o in ((kk_h, b_h, w, nw, left), (kk_v, b_v, h, nh, top)):
        assert (b[:, 0] >= 0).all() and (b[:, 0] + b[:, 1] <= n_in).all() and (b[:, 1] <= kk.shape[1]).all()
        sums = kk.astype(np.int64).sum(1)
        assert (np.abs(sums - (1 << 22)) < 64).all()
        if n_out <= 4000:
            fk, fb = pil_bicubic_tables(n_in, n_out)
            assert np.array_equal(fk[o:o + S], kk) and np.array_equal(fb[o:o + S], b)
        else:
            pk, pb = pil_bicubic_rows(n_in, n_out, o + 100, o + 110)
            assert np.array_equal(pk, kk[100:110]) and np.array_equal(pb, b[100:110])
    assert vmin == b_v[:, 0].min() and vmin + rows == (b_v[:, 0] + b_v[:, 1]).max() <= h
    if h != nh:
        assert ks_v == 2 * int(np.ceil(2.0 * max(h / nh, 1.0))) + 1


def test_ragged_plan_small_output_of_a_large_image():
    from lemon_amd.data import ragged_plan
    hdr, _ = ragged_plan(8000, 6000, 30)            # 801 vertical taps per output row: one row per vertical block
    assert int(hdr[7]) == 801 and int(hdr[8]) == 4096 // 803


def test_ragged_prefixes_and_selection_share_the_buffer():
    import torch
    from lemon_amd.data import RaggedImages, RaggedPlans, ragged_plan
    shapes = [(32, 32), (640, 480), (2, 300), (640, 480)]
    plans = RaggedPlans(dict.fromkeys(shapes))
    desc, off = [], 0
    for h, w in shapes:
        desc.append((off, h, w, plans.shapes.index((h, w))))
        off += h * w * 3
    r = RaggedImages(torch.zeros(off, dtype=torch.uint8), np.array(desc), plans)
    assert len(r) == 4 and r.shape == (4,)
    sub = r[torch.tensor([3, 0])]
    assert sub.data is r.data and sub.plans is r.plans and np.array_equal(sub.desc, r.desc[[3, 0]])
    assert np.array_equal(r[1:3].desc, r.desc[1:3])
    hdr = [ragged_plan(h, w, 224)[0] for h, w in shapes]
    assert int(hdr[0][11]) == 32 and int(hdr[0][12]) == 2                   # up-sampled: every input row, 16 per block
    assert 224 < int(hdr[1][11]) < 640 and int(hdr[1][12]) == -(-int(hdr[1][11]) // 16)   # the crop window's rows only


def _scalar_rows(in_size, out_size, lo, hi):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for BICUBIC, one output index at a time (the recipe
    data.pil_bicubic_rows vectorises)."""
    import math

    def bicubic(x):
        a = -0.5
        x = -x if x < 0.0 else x
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0
    scale = filterscale = in_size / out_size
    filterscale = max(filterscale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    kk, bounds, ss = np.zeros((hi - lo, ksize), np.int32), np.zeros((hi - lo, 2), np.int32), 1.0 / filterscale
    for xx in range(lo, hi):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx - lo, x] = int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22))
        bounds[xx - lo] = (xmin, xmax)
    return kk, bounds


def test_vectorised_tap_rows_equal_the_scalar_recipe():
    from lemon_amd.data import pil_bicubic_rows
    rng = np.random.default_rng(4)
    cases = [(32, 224), (300, 33600), (2, 224), (8000, 298), (6000, 224), (480, 224), (225, 224), (37, 91), (91, 30)]
    cases += [(int(rng.integers(2, 9000)), int(rng.integers(30, 3000))) for _ in range(60)]
    for i, o in cases:
        if i == o:
            continue
        lo = max(0, o // 2 - 112)
        hi = min(o, lo + 224)
        a, b = _scalar_rows(i, o, lo, hi), pil_bicubic_rows(i, o, lo, hi)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (i, o)
