"""GPU: file-backed image datasets -- lemon_preprocess_ragged (images of different sizes in one launch) against the PIL + torch
generic_transform, sub-batch selection, the decode pool -> ragged batch -> encoder path, and the CLI from image files with the
pool and with the in-process thread path (LEMON_DECODE_WORKERS=0)."""
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(32, 32), (37, 91), (224, 224), (225, 224), (640, 480), (480, 640), (640, 480), (3000, 2000), (100, 3000),
          (8000, 6000), (37, 91)]


@pytest.fixture(scope="module")
def ragged_case():
    from lemon_amd.data import RaggedImages, generic_transform
    rng = np.random.default_rng(11)
    imgs = []
    for h, w in SHAPES:            # smooth content plus noise (the taps see gradients and clipping); uint8 noise alone when large
        if h * w > 1 << 20:
            imgs.append(rng.integers(0, 256, (h, w, 3), dtype=np.uint8))
            continue
        yy, xx = np.mgrid[0:h, 0:w]
        base = (128 + 100 * np.sin(yy[..., None] / (3.0 + h / 50) + xx[..., None] / (5.0 + w / 70) + np.arange(3))).astype(np.int16)
        imgs.append(np.clip(base + rng.integers(-60, 61, (h, w, 3)), 0, 255).astype(np.uint8))
    ref = {S: torch.stack([generic_transform(Image.fromarray(a), S) for a in imgs]) for S in (224, 30)}
    return imgs, RaggedImages.from_arrays(imgs, "cuda"), ref


def test_ragged_transform_bit_identical_to_pil(hip, ragged_case):
    from lemon_amd.data import gpu_transform_ragged
    imgs, r, ref = ragged_case
    B = len(imgs)
    got = gpu_transform_ragged(r, 224).cpu()
    assert got.shape == (B, 3, 224, 224)
    for i in range(B):
        assert torch.equal(got[i], ref[224][i]), (SHAPES[i], (got[i] - ref[224][i]).abs().max())
    pm = gpu_transform_ragged(r, 224, patch=16).cpu()
    assert torch.equal(pm, ref[224].view(B, 3, 14, 16, 14, 16).permute(0, 2, 4, 1, 3, 5).reshape(B, 196, 768))
    # an output size that is not a multiple of 4 (one pixel per lane), with and without patches
    assert torch.equal(gpu_transform_ragged(r, 30).cpu(), ref[30])
    assert torch.equal(gpu_transform_ragged(r, 30, patch=6).cpu(), ref[30].view(B, 3, 5, 6, 5, 6).permute(0, 2, 4, 1, 3, 5).reshape(B, 25, 108))


def test_ragged_operand_equals_same_shape_operand(hip, ragged_case):
    from lemon_amd.data import gpu_transform_batch, gpu_transform_ragged
    from lemon_amd.ops import split_operand, unpack_act_t
    imgs, r, ref = ragged_case
    B, P = len(imgs), 32
    po = gpu_transform_ragged(r, 224, patch=P, operand=True)
    nP, K = po.n_patches, po.k
    rows = unpack_act_t(po.at, B * nP, K).view(B, nP, K)
    # every image: exactly the fp16 split of its fp32 patch rows
    pm = gpu_transform_ragged(r, 224, patch=P)
    y3 = split_operand(pm.reshape(B * nP, K), "f16x3").view(B, nP, 3, K)
    assert torch.equal(rows, y3[:, :, 0].float() + y3[:, :, 2].float() * (1.0 / 2048.0))
    # per same-shape group: the rows the same-shape kernel writes (where its LDS tile holds the image's windows)
    groups = {}
    for i, s in enumerate(SHAPES):
        groups.setdefault(s, []).append(i)
    checked = 0
    for (h, w), idx in groups.items():
        try:
            g = gpu_transform_batch(torch.from_numpy(np.stack([imgs[i] for i in idx])).cuda(), 224, patch=P, operand=True)
        except ValueError:
            assert h * w >= 3000 * 2000         # only the large images exceed the same-shape kernel
            continue
        assert torch.equal(unpack_act_t(g.at, len(idx) * nP, K).view(len(idx), nP, K), rows[idx])
        checked += 1
    assert checked >= 6


def test_ragged_selection_gives_the_rows_of_the_full_batch(hip, ragged_case):
    from lemon_amd.data import gpu_transform_ragged
    imgs, r, ref = ragged_case
    full = gpu_transform_ragged(r, 224, patch=32)
    sel = torch.tensor([9, 0, 4, 4, 7, 2])
    sub = r[sel]
    assert len(sub) == 6 and sub.data is r.data
    assert torch.equal(gpu_transform_ragged(sub, 224, patch=32), full[sel.cuda()])
    assert torch.equal(gpu_transform_ragged(r[3:6], 224, patch=32), full[3:6])
    assert gpu_transform_ragged(r[0:0], 224).shape == (0, 3, 224, 224)


def _write_files(d, n_jpg=64):
    rng = np.random.default_rng(5)
    sizes = [(480, 640), (427, 640), (375, 500), (612, 612), (64, 80)]
    paths = []
    for i in range(n_jpg):
        h, w = sizes[i % len(sizes)]
        yy, xx = np.mgrid[0:h, 0:w]
        px = np.clip(128 + 90 * np.sin(yy[..., None] / 17.0 + xx[..., None] / (9.0 + i) + np.arange(3) * i)
                     + rng.integers(-30, 31, (h, w, 3)), 0, 255).astype(np.uint8)
        p = os.path.join(d, f"{i:03d}.jpg")
        Image.fromarray(px).save(p, quality=90, subsampling=2)
        paths.append(p)
    p = os.path.join(d, "extra.png")
    Image.fromarray(rng.integers(0, 256, (90, 70, 4), dtype=np.uint8), "RGBA").save(p)
    paths.insert(17, p)
    return paths


def test_files_through_pool_and_ragged_batches_embed_like_pil(hip, tmp_path, arch="tiny"):
    # (the operand form of the hand-written GEMM is covered end to end by the CLI test below: ViT-B/32)
    from lemon_amd.clip import ClipConfig, LemonCLIP
    from lemon_amd.data import ImageLabelSet, RaggedImages, generic_transform
    from lemon_amd.pipeline import Embedder
    paths = _write_files(str(tmp_path))
    n = len(paths)
    cfg = ClipConfig.named(arch)
    torch.manual_seed(0)
    emb = Embedder(LemonCLIP(cfg), torch.device("cuda"), batch_size=24)
    dset = ImageLabelSet(paths, list(range(n)), list(range(n)), image_size=cfg.image_size)
    got, seen = [], []
    for px, clean, noisy in dset.batches(30, 3, n, device="cuda"):
        assert isinstance(px, RaggedImages) and len(px) == len(clean) == len(noisy)
        seen += list(noisy)
        got.append(emb.embed_images(px))
    emb.raise_if_nonfinite()
    assert seen == list(range(3, n))
    got = torch.cat(got)
    ref_px = torch.stack([generic_transform(Image.open(p).convert("RGB"), cfg.image_size) for p in paths[3:]])
    ref = emb.embed_images(ref_px)
    assert got.shape == ref.shape
    assert float((got - ref).abs().max()) < 5e-6


def _mscoco_dir(root, n=96):
    from lemon_amd.data import synthetic_caption_frame
    df, _ = synthetic_caption_frame(n, 3)
    os.makedirs(os.path.join(root, "synthetic"))
    rng = np.random.default_rng(7)
    sizes = [(480, 640), (640, 480), (427, 640), (375, 500), (612, 612), (1200, 1600)]
    for j, fn in enumerate(df["filename"]):
        h, w = sizes[j % len(sizes)] if j % 23 else (1200, 1600)
        h, w = (h // 2, w // 2) if j % 5 else (h, w)
        px = np.clip(rng.integers(0, 256, (1, 1, 3)) + rng.integers(-40, 41, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(px).save(os.path.join(root, "synthetic", fn), quality=90, subsampling=2)
    df.to_pickle(os.path.join(root, "multimodal_mislabel_split.pkl"))


def test_cli_from_image_files_pool_equals_thread_path(hip, tmp_path):
    data = str(tmp_path / "coco")
    _mscoco_dir(data)
    res = {}
    for mode, workers in (("pool", None), ("threads", "0")):
        env = dict(os.environ)
        env.pop("LEMON_DECODE_WORKERS", None)
        if workers is not None:
            env["LEMON_DECODE_WORKERS"] = workers
        out = str(tmp_path / mode)
        cmd = ["timeout", "-k", "10", "400", sys.executable, "-m", "lemon_amd.run_lemon", "--output_dir", out, "--dataset", "mscoco",
               "--noise_type", "random", "--noise_level", "0.4", "--data_root", data, "--clip_path", "random", "--knn_k", "5",
               "--skip_hparam_optim", "--encoder_batch", "64"]
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
        assert r.returncode == 0, (mode, r.stdout[-3000:], r.stderr[-3000:])
        res[mode] = pickle.load(open(os.path.join(out, "res.pkl"), "rb"))["df"]
    a, b = res["pool"], res["threads"]
    assert len(a) == len(b) > 60
    for col in ("sset", "idx", "actual_label", "actual_label_text", "noisy_label", "noisy_label_text", "is_mislabel",
                "is_correct_label"):
        assert list(a[col]) == list(b[col]), col
    # the per-sample quantities the scores are made of: image-caption distance and the neighbour distances of both modalities
    for col in ("d_1", "D_n", "D_m"):
        va, vb = np.stack(a[col].values).astype(np.float64), np.stack(b[col].values).astype(np.float64)
        assert np.isfinite(va).all() and float(np.abs(va - vb).max()) < 1e-4, col
