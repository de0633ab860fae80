"""GPU: baseline JPEGs decoded on the device (lemon_jpeg_decode after the host's Huffman pass) against PIL, bit for bit: the
public decode_jpegs, the file batches of ImageLabelSet in both LEMON_JPEG modes, and the CLI in both modes."""
import io
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

from tests import jpegfx
from tests.test_gpu_file_pipeline import _mscoco_dir, _write_files

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POISON = 0xA5


def _pil(raw):
    return np.asarray(Image.open(io.BytesIO(raw)).convert("RGB"))


def test_device_decode_equals_pil_in_one_mixed_batch_with_poisoned_buffers(hip, tmp_path):
    from lemon_amd.data import RaggedImages, decode_jpegs
    cases = jpegfx.accepted_cases()
    raws = [c[1] for c in cases]
    paths = jpegfx.write_all(str(tmp_path), cases[:5])
    files = paths + raws[5:]                      # paths and bytes objects alike
    r = decode_jpegs(files, "cuda", poison=POISON)
    assert isinstance(r, RaggedImages) and len(r) == len(cases) and r.layout.n_jpeg == len(cases)
    torch.cuda.synchronize()
    data = r.data.cpu().numpy()
    covered = np.zeros(data.size, bool)
    covered[:r.layout.decoded_off] = True         # the copied payload: records and the aux table
    for i, (name, raw) in enumerate(cases):
        ref = _pil(raw)
        o, h, w, _ = (int(v) for v in r.desc[i])
        assert (h, w) == ref.shape[:2] and o >= r.layout.decoded_off, name
        got = data[o:o + h * w * 3].reshape(h, w, 3)
        assert np.array_equal(got, ref), (name, int(np.abs(got.astype(int) - ref).max()), int((got != ref).sum()))
        assert np.array_equal(r.image(i).cpu().numpy(), ref), name
        assert not covered[o:o + h * w * 3].any(), name
        covered[o:o + h * w * 3] = True
    assert (data[~covered] == POISON).all()       # nothing written between or after the images
    assert (~covered).sum() > 0


def test_decode_jpegs_raises_for_a_declined_file_unless_fallback(hip):
    from lemon_amd.data import decode_jpegs
    good = jpegfx.accepted_cases()[3][1]
    for name, raw, pil_ok in jpegfx.declined_cases():
        with pytest.raises(ValueError, match="not decodable on the GPU"):
            decode_jpegs([good, raw], "cuda")
        if pil_ok:
            r = decode_jpegs([good, raw, good], "cuda", fallback=True)
            assert r.layout.n_jpeg == 2
            for i, x in enumerate((good, raw, good)):
                assert np.array_equal(r.image(i).cpu().numpy(), _pil(x)), (name, i)
        else:
            with pytest.raises(Exception) as e:          # PIL's own exception for a corrupt file
                decode_jpegs([good, raw], "cuda", fallback=True)
            assert not isinstance(e.value, ValueError) or "not decodable on the GPU" not in str(e.value)
    with pytest.raises(TypeError):
        decode_jpegs([good], "cpu")
    assert len(decode_jpegs([], "cuda")) == 0


def _same(x, y):
    ax, ay = np.asarray(x), np.asarray(y)
    if ax.dtype.kind in "fc":
        return np.array_equal(ax, ay, equal_nan=True)
    return np.array_equal(ax, ay)


def _extra_files(d):
    rng = np.random.default_rng(9)
    extra = []
    p = os.path.join(d, "progressive.jpg")
    Image.fromarray(jpegfx.pixels(300, 260, rng)).save(p, quality=90, progressive=True)
    extra.append(p)
    p = os.path.join(d, "gray.jpg")
    Image.fromarray(jpegfx.pixels(320, 240, rng, channels=1)).save(p, quality=90)
    extra.append(p)
    return extra


def test_file_batches_equal_the_pil_mode_bit_for_bit(hip, tmp_path, monkeypatch):
    from lemon_amd.clip import ClipConfig, LemonCLIP
    from lemon_amd.data import ImageLabelSet, RaggedImages
    from lemon_amd.pipeline import Embedder
    paths = _write_files(str(tmp_path))
    extra = _extra_files(str(tmp_path))
    paths[5:5] = extra[:1]
    paths.append(extra[1])
    n = len(paths)
    cfg = ClipConfig.named("tiny")
    torch.manual_seed(0)
    emb = Embedder(LemonCLIP(cfg), torch.device("cuda"), batch_size=24)
    dset = ImageLabelSet(paths, list(range(n)), list(range(n)), image_size=cfg.image_size)
    res = {}
    for mode in ("pil", "gpu"):
        monkeypatch.setenv("LEMON_JPEG", mode)
        imgs, embs, seen = [], [], []
        for px, clean, noisy in dset.batches(30, 0, n, device="cuda"):
            assert isinstance(px, RaggedImages) and len(px) == len(noisy)
            seen += list(noisy)
            imgs += [px.image(i).cpu() for i in range(len(px))]
            embs.append(emb.embed_images(px))
        emb.raise_if_nonfinite()
        assert seen == list(range(n))
        res[mode] = (imgs, torch.cat(embs))
    for i, p in enumerate(paths):
        ref = torch.from_numpy(np.asarray(Image.open(p).convert("RGB")).copy())
        assert torch.equal(res["gpu"][0][i], res["pil"][0][i]), p
        assert torch.equal(res["gpu"][0][i], ref), p
    assert torch.equal(res["gpu"][1], res["pil"][1])


def test_cli_from_image_files_gpu_jpeg_equals_pil_mode(hip, tmp_path):
    data = str(tmp_path / "coco")
    _mscoco_dir(data)
    res = {}
    for mode in ("gpu", "pil"):
        env = dict(os.environ, LEMON_JPEG=mode)
        env.pop("LEMON_DECODE_WORKERS", None)
        out = str(tmp_path / mode)
        cmd = ["timeout", "-k", "10", "400", sys.executable, "-m", "lemon_amd.run_lemon", "--output_dir", out, "--dataset", "mscoco",
               "--noise_type", "random", "--noise_level", "0.4", "--data_root", data, "--clip_path", "random", "--knn_k", "5",
               "--skip_hparam_optim", "--encoder_batch", "64"]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)     # a fresh child process per mode
        assert r.returncode == 0, (mode, r.stdout[-3000:], r.stderr[-3000:])
        res[mode] = pickle.load(open(os.path.join(out, "res.pkl"), "rb"))["df"]
    a, b = res["gpu"], res["pil"]
    assert len(a) == len(b) > 60 and list(a.columns) == list(b.columns)
    for col in a.columns:
        for x, y in zip(a[col].values, b[col].values):
            assert _same(x, y), (col, x, y)
