"""python -m lemon_amd.deepknn_baseline -- the deep-kNN label-error baseline of the reference's
`python -m lib.baselines.run_deepknn` (lib/baselines/run_deepknn.py), LEMoN's main competitor.

The reference script drives a module (`MMNB`) that is missing upstream, so only what has a defined meaning without it is
built: the flags of run_deepknn.py:44-115 that select data, noise, encoder, metric, k and the number of text clusters, the
label construction (class ids, or -- caption datasets -- k-means cluster ids of the noisy train sentences,
get_dataset(..., cluster_text=True), :158-166) and the `--dist_method deep_knn` score itself: the fraction of a sample's k
nearest TRAIN images (self excluded on the train split) whose noisy label differs from the sample's.  Flags whose meaning
lives only in the missing module (--agg_type, --dist_method other than deep_knn, --deep_knn_thres) are accepted and refused
when set away from their default.

Outputs (:141-142,266-276): args.json, dists.npy (one score per sample, splits in the order train, test, val), label_flips_all.npy
(is_mislabel per sample, same order; the reference saves the same values grouped by DataLoader batch), datasplit.npy,
len_splits.npy (batches per split), runtime.npy, done; AUROC / AUPRC per split are printed."""
import argparse
import os
import sys
import time

import numpy as np
import torch

from .cli_common import add_extension_flags

UNDEFINED_DEFAULTS = {"agg_type": "mean", "dist_method": "deep_knn", "deep_knn_thres": 0.5}


def build_parser():
    p = argparse.ArgumentParser(description="Deep-kNN label-error baseline (run_deepknn.py) on class or text-cluster labels")
    p.add_argument("--exp_name", type=str, default="pretrain")
    p.add_argument("--dataset", type=str, default="cifar10",
                   choices=["cifar10", "cifar100", "mscoco", "flickr30k", "mmimdb", "mimiccxr_caption", "stanford_cars",
                            "mini_imagenet", "cc3m", "cifar10_full", "cifar100_full"])
    p.add_argument("--algorithm", type=str, default="huggingface_clip", choices=["huggingface_clip", "biomed_clip"])
    p.add_argument("--data_dir", dest="data_root", type=str, default=argparse.SUPPRESS, help="alias of --data_root")
    p.add_argument("--output_dir", type=str, required=True)
    p.add_argument("--seed", type=int, default=0, help="seed of the data split, the noise and everything else")
    p.add_argument("--flip_type", type=str, default="real")
    p.add_argument("--batch_size", default=258, type=int)
    p.add_argument("--percent_flips", type=float, default=0.3)
    p.add_argument("--noise_labels", action="store_true")
    p.add_argument("--dist_type", type=str, default="cosine", choices=["cosine", "euclidean"])
    p.add_argument("--val_only", action="store_true")
    p.add_argument("--knn_k", type=int, default=10)
    p.add_argument("--num_text_clusters", type=int, default=100)
    p.add_argument("--agg_type", type=str, default="mean", choices=["mean", "sum", "median", "max"])
    p.add_argument("--dist_method", type=str, default="deep_knn",
                   choices=["nn_pairwise", "nn_ot", "single_pairwise", "deep_knn", "nn_pairwise_multimodal"])
    p.add_argument("--deep_knn_thres", type=float, default=0.5)
    p.add_argument("--debug", action="store_true", help="no out.txt / err.txt copies of the console")
    add_extension_flags(p)
    return p


def check_defined(args):
    """The flags that only the reference's missing MMNB module gives a meaning: refuse anything but their default."""
    for name, default in UNDEFINED_DEFAULTS.items():
        if getattr(args, name) != default:
            raise NotImplementedError(f"--{name} {getattr(args, name)}: its meaning is defined only by the reference's MMNB module, "
                                      f"which is missing upstream; only the default ({default}) is accepted")
    if not args.noise_labels:
        raise NotImplementedError("run_deepknn.py:245-246 raises without --noise_labels: the baseline scores the NOISY labels")


def main(argv=None):
    from .cli_common import run_with_tee
    args = build_parser().parse_args(argv)
    check_defined(args)
    return run_with_tee(_run, args)


def _run(args):
    from . import metrics as M
    from .baselines import deep_knn_scores
    from .cli_common import prepare
    from .data import CAPTION_DATASETS, cluster_text_labels
    from .index import IndexFlatIP, IndexFlatL2

    # the names cli_common.prepare reads (run_lemon.py's)
    args.clip_model, args.noise_type, args.noise_level, args.data_seed = args.algorithm, args.flip_type, args.percent_flips, args.seed
    args.custom_cifar_prompt, args.compr_dataset_size_limit = None, 1 << 62       # the DB is the whole train split
    ctx = prepare(args)
    if ctx.world > 1:
        raise NotImplementedError("deepknn_baseline runs on one device")
    device, sets = ctx.device, ctx.sets
    start = time.time()
    if args.dataset in CAPTION_DATASETS:
        _, (tr, va, te) = cluster_text_labels((sets["train"], sets["val"], sets["test"]), ctx.embedder, ctx.tokenize,
                                              n_clusters=args.num_text_clusters)
        labels = {"train": tr, "val": va, "test": te}
    else:
        labels = sets
    e_train = ctx.embed_split(sets["train"], "train")[0]
    index = (IndexFlatIP if args.dist_type == "cosine" else IndexFlatL2)(e_train.shape[1], device)
    index.add(e_train)
    db_label = np.asarray(labels["train"].noisy).astype(np.int32)
    dists, flips, splits, len_splits = [], [], [], []
    for phase in (["test", "val"] if args.val_only else ["train", "test", "val"]):
        e_img = e_train if phase == "train" else ctx.embed_split(sets[phase], phase)[0]
        noisy, clean = np.asarray(labels[phase].noisy), np.asarray(labels[phase].clean)
        score = deep_knn_scores(index, e_img, noisy.astype(np.int32), db_label, args.knn_k, is_train=(phase == "train"))
        score = score.cpu().numpy()
        flip = 1 - (clean == noisy).astype(np.int64)
        dists.append(score); flips.append(flip); splits.append(np.array([phase] * len(flip)))
        len_splits.append((len(flip) + args.batch_size - 1) // args.batch_size)
        if 0 < flip.sum() < len(flip):
            m = M.prob_metrics(flip, score)
            print(f"{phase}: AUROC {m['AUROC']:.4f}  AUPRC {m['AUPRC']:.4f}")
    torch.cuda.synchronize(device)
    out = str(ctx.out_dir)
    np.save(os.path.join(out, "runtime.npy"), np.array([time.time() - start]))
    np.save(os.path.join(out, "len_splits.npy"), np.array(len_splits))
    np.save(os.path.join(out, "label_flips_all.npy"), np.concatenate(flips))
    np.save(os.path.join(out, "dists.npy"), np.concatenate(dists))
    np.save(os.path.join(out, "datasplit.npy"), np.concatenate(splits))
    with open(os.path.join(out, "done"), "w") as f:
        f.write("done")
    return 0


if __name__ == "__main__":
    sys.exit(main())
