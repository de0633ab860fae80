"""GPU: PNGs unfiltered and expanded on the device (lemon_png_decode behind the workers' chunk walk and inflate) against PIL, bit
for bit: the public decode_pngs on the shape x colour-type x filter matrix with poisoned buffers, the host twin, the two device
verdicts, and the file batches of the loader in both LEMON_PNG modes, composed with the LEMON_JPEG modes."""
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpegfx, pngfx

pytestmark = pytest.mark.gpu

POISON = 0xA5


@pytest.fixture(scope="module")
def accepted():
    return pngfx.accepted_cases()


def test_device_decode_equals_pil_and_the_host_twin_in_one_mixed_batch_with_poisoned_buffers(hip, tmp_path, accepted):
    from lemon_amd import png_host
    from lemon_amd.data import RaggedImages, decode_pngs
    raws = [c[1] for c in accepted]
    paths = pngfx.write_all(str(tmp_path), accepted[:5])
    files = paths + raws[5:]                      # paths and bytes objects alike
    r = decode_pngs(files, "cuda", poison=POISON)
    assert isinstance(r, RaggedImages) and len(r) == len(accepted) and r.layout.n_png == len(accepted) and not r.status.any()
    torch.cuda.synchronize()
    data = r.data.cpu().numpy()
    covered = np.zeros(data.size, bool)
    covered[:r.layout.png_decoded_off] = True     # the copied payload: records and the aux table
    for i, (name, raw) in enumerate(accepted):
        ref = pngfx.pil_rgb(raw)
        o, h, w, _ = (int(v) for v in r.desc[i])
        assert (h, w) == ref.shape[:2] and o >= r.layout.png_decoded_off, name
        got = data[o:o + h * w * 3].reshape(h, w, 3)
        assert np.array_equal(got, ref), (name, int((got != ref).sum()))
        twin, st = png_host.decode_host(png_host.decode_record(raw)[0])
        assert st == 0 and np.array_equal(got, twin), name
        assert not covered[o:o + h * w * 3].any(), name
        covered[o:o + h * w * 3] = True
    assert (data[~covered] == POISON).all()       # every image's neighbours in the packed buffer: untouched
    assert (~covered).sum() > 0


def test_filter_and_index_verdicts_land_on_exactly_those_images(hip):
    from lemon_amd import png_host
    from lemon_amd.data import decode_pngs
    rng = np.random.default_rng(21)
    good = [pngfx.png_bytes(pngfx.pixels(h, w, ct, rng), ct, plte=pngfx.palette(256, rng) if ct == 3 else None)
            for h, w, ct in ((70, 33, 2), (9, 65, 0), (66, 17, 3), (130, 20, 6))]
    filters = [r % 5 for r in range(70)]
    filters[65] = 5
    bad_filter = pngfx.png_bytes(pngfx.pixels(70, 21, 4, rng), 4, filters)
    plte = pngfx.palette(4, rng)
    idx = pngfx.pixels(67, 19, 3, rng, plte_count=4)
    idx[66, 18] = 4
    bad_index = pngfx.png_bytes(idx, 3, plte=plte)
    files = [good[0], bad_filter, good[1], good[2], bad_index, good[3]]
    # the launch itself: statuses on exactly those two, the others exact, nothing written outside the images' own regions
    from lemon_amd.data import launch_png_decode
    from lemon_amd.jpeg_host import BatchLayout
    lay, off, recs = BatchLayout(), 0, []
    for raw in files:
        rec, _ = png_host.decode_record(raw)
        lay.add_png_record(off, rec)
        recs.append((off, rec.data))
        off = (off + rec.data.nbytes + 15) & ~15
    aux = lay.finish(off)
    host = np.zeros(lay.payload_bytes, np.uint8)
    for o, a in recs:
        host[o:o + a.size] = a
    host[lay.aux_off:] = aux.view(np.uint8)
    data = torch.empty(lay.total_bytes + 64, dtype=torch.uint8, device="cuda")
    data[:host.size] = torch.from_numpy(host).cuda()
    status = launch_png_decode(data, lay, poison=POISON).cpu().numpy()
    assert list(status) == [0, png_host.FILTER, 0, 0, png_host.INDEX, 0]
    out = data.cpu().numpy()
    inside = np.zeros(out.size, bool)
    inside[:lay.png_decoded_off] = True
    for i, raw in enumerate(files):
        o, h, w, _ = lay.desc[i]
        inside[o:o + h * w * 3] = True
        if status[i] == 0:
            assert np.array_equal(out[o:o + h * w * 3].reshape(h, w, 3), pngfx.pil_rgb(raw)), i
    assert (out[~inside] == POISON).all() and np.array_equal(out[:host.size], host)
    with pytest.raises(ValueError, match="filter type above 4"):
        decode_pngs(files, "cuda")
    with pytest.raises(ValueError, match="palette index beyond PLTE"):
        decode_pngs(files[2:], "cuda")
    with pytest.raises(OSError):                  # fallback: PIL's own exception for the filter byte
        decode_pngs(files, "cuda", fallback=True)
    files.pop(1)
    r = decode_pngs(files, "cuda", fallback=True, poison=POISON)
    assert list(r.status) == [0, 0, 0, png_host.INDEX, 0]
    for i, raw in enumerate(files):
        assert np.array_equal(r.image(i).cpu().numpy(), pngfx.pil_rgb(raw)), i
    # a file the host declines: ValueError naming the status, or PIL's pixels
    depth16 = pngfx.declined_cases()[0][1]
    with pytest.raises(ValueError, match="not 8-bit"):
        decode_pngs([good[0], depth16], "cuda")
    r = decode_pngs([good[0], depth16, good[1]], "cuda", fallback=True)
    assert r.layout.n_png == 2
    for i, raw in enumerate((good[0], depth16, good[1])):
        assert np.array_equal(r.image(i).cpu().numpy(), pngfx.pil_rgb(raw)), i
    with pytest.raises(TypeError):
        decode_pngs([good[0]], "cpu")
    assert len(decode_pngs([], "cuda")) == 0


def _mixed_directory(d):
    """About 40 files: PNGs of every colour type, baseline JPEGs, PNGs the host declines, one PNG the device declines."""
    rng = np.random.default_rng(31)
    files, n_records = [], 0
    for k in range(22):
        ct = pngfx.COLOUR_TYPES[k % 5]
        h, w = int(rng.integers(20, 131)), int(rng.integers(20, 131))
        n = int(rng.integers(2, 257))
        files.append((f"p{k:02d}.png", pngfx.png_bytes(pngfx.pixels(h, w, ct, rng, "smooth" if k % 2 else "random", n), ct,
                                                       list(rng.integers(0, 5, h)), plte=pngfx.palette(n, rng) if ct == 3 else None,
                                                       splits=None if k % 3 else 100)))
        n_records += 1
    for k in range(10):
        files.append((f"j{k:02d}.jpg", jpegfx.jpeg_bytes(jpegfx.pixels(int(rng.integers(24, 120)), int(rng.integers(24, 120)), rng),
                                                         quality=85, subsampling=k % 3)))
    declined = [c for c in pngfx.declined_cases() if c[0] in ("depth16", "depth1", "depth4", "crc_idat", "stream_long", "actl")]
    files += [(f"d_{c[0]}.png", c[1]) for c in declined]
    idx = pngfx.pixels(40, 50, 3, rng, plte_count=3)
    idx[7, 7] = 3
    files.append(("x_index.png", pngfx.png_bytes(idx, 3, plte=pngfx.palette(3, rng))))
    n_records += 1
    order = rng.permutation(len(files))
    paths = []
    for i in order:
        p = os.path.join(d, files[i][0])
        with open(p, "wb") as fh:
            fh.write(files[i][1])
        paths.append(p)
    return paths, n_records, 1


@pytest.mark.parametrize("jpeg_mode", ["pil", "gpu"])
def test_file_batches_with_device_png_equal_the_pil_mode(hip, tmp_path, monkeypatch, jpeg_mode):
    from lemon_amd.data import gpu_transform_ragged
    from lemon_amd.loader import ragged_batches
    paths, n_records, n_fallback = _mixed_directory(str(tmp_path))
    assert 36 <= len(paths) <= 44
    monkeypatch.setenv("LEMON_JPEG", jpeg_mode)
    res = {}
    for mode in ("pil", "gpu"):
        monkeypatch.setenv("LEMON_PNG", mode)
        stats, imgs, feats = {}, [], []
        for s, e, px in ragged_batches(paths, 16, 0, len(paths), "cuda", workers=2, ring_bytes=8 << 20, stats=stats):
            imgs += [px.image(i).cpu() for i in range(len(px))]
            feats.append(gpu_transform_ragged(px, 32).cpu())
        res[mode] = (imgs, torch.cat(feats), stats)
    for i, p in enumerate(paths):
        ref = torch.from_numpy(np.asarray(Image.open(p).convert("RGB")).copy())
        assert torch.equal(res["gpu"][0][i], ref) and torch.equal(res["pil"][0][i], ref), p
    assert torch.equal(res["gpu"][1], res["pil"][1])
    assert res["gpu"][2]["png_records"] == n_records and res["gpu"][2]["png_fallback"] == n_fallback
    assert "png_records" not in res["pil"][2] and "png_fallback" not in res["pil"][2]
    assert res["gpu"][2].get("jpeg_images", 0) == res["pil"][2].get("jpeg_images", 0) == (10 if jpeg_mode == "gpu" else 0)


def test_without_lemon_png_no_worker_emits_a_png_record(hip, tmp_path, monkeypatch):
    from lemon_amd import png_host
    from lemon_amd.loader import DecodePool, ragged_batches
    monkeypatch.delenv("LEMON_PNG", raising=False)
    monkeypatch.delenv("LEMON_JPEG", raising=False)
    paths = pngfx.write_all(str(tmp_path), pngfx.accepted_cases()[:8])
    seen = []

    class Spy(DecodePool):
        def images(self, lo=0, hi=None):
            assert self.png is False
            for i, a in super().images(lo, hi):
                seen.append(type(a))
                yield i, a

    monkeypatch.setattr("lemon_amd.loader.DecodePool", Spy)
    stats = {}
    n = sum(len(px) for _, _, px in ragged_batches(paths, 4, 0, len(paths), "cuda", workers=1, ring_bytes=1 << 20, stats=stats))
    assert n == 8 and len(seen) == 8 and png_host.PngRecord not in seen and all(t is np.ndarray for t in seen)
    assert "png_records" not in stats
