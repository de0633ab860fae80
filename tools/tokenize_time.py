"""Times caption tokenization: the host tokenizers (lemon_amd/tokenizer.py, the default path) against their device form
(LEMON_TOKENIZE=device: tokenizer.device_form -> lemon_tokenize), and both against the text tower that consumes the ids.

    python tools/tokenize_time.py --out profiles/tokenize [--merges bpe_simple_vocab_16e6.txt.gz] [--vocab vocab.txt]

Two seeded corpora of printable-ASCII text over the words of tests/golden/tokenizer.npz:
  clip  200 000 captions of 8 .. 77 tokens, CLIP BPE at context 77 (merges: --merges, else the fixture's sparse table), text tower
        of ViT-B/32;
  bert  20 000 reports that fill the 256-token context, WordPiece (vocabulary: --vocab, else pieces of the corpus's own words),
        the BiomedCLIP text tower.
Per corpus, captions/s of
  host    the Python tokenizer, word cache warm, on the first --host_rows rows (it is a per-row loop: the rate does not depend
          on the row count);
  device  the device form on the whole corpus in calls of --batch rows: pack, one upload, the kernel, the length / status
          read-back, declined rows filled on the host (none in these corpora);
  tower   Embedder.embed_texts on device ids of --tower_rows rows, de-duplication off.
Every figure is the median of --passes timed passes after one warm-up pass (host clock around work that ends in a device
synchronise); all passes go to <out>/tokenize_time.json.  The ids of the two paths are compared before anything is timed."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def words_and_merges():
    import numpy as np
    fx = np.load(os.path.join(ROOT, "tests", "golden", "tokenizer.npz"))
    words = sorted({w.lower() for t in fx["texts"] for w in str(t).replace("_", " ").replace(".", " ").split() if w.isascii() and w.isalpha()})
    ranks = {(str(a), str(b)): int(r) for a, b, r in zip(fx["merge_first"], fx["merge_second"], fx["merge_rank"])}
    return words, ranks


def make_corpus(words, n, lo, hi, seed):
    """n captions of lo .. hi words, some capitalised, a comma or a full stop now and then (a punctuation mark is a token)"""
    import numpy as np
    rs = np.random.RandomState(seed)
    out = []
    for count in rs.randint(lo, hi + 1, n):
        pick = rs.randint(0, len(words), count)
        marks = rs.randint(0, 12, count)
        out.append(" ".join(words[p].capitalize() if m == 0 else words[p] + "," if m == 1 else words[p] + "." if m == 2 else words[p]
                            for p, m in zip(pick, marks)))
    return out


def piece_vocab(words):
    toks = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]", ",", "."]
    for w in words:
        cut = max(1, len(w) // 2)
        toks += [w[:cut], "##" + w[cut:]] if len(w) > 3 else [w]
    return list(dict.fromkeys(t for t in toks if t != "##"))


def timed(fn, passes, sync):
    fn()
    sync()
    out = []
    for _ in range(passes):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join("profiles", "tokenize"))
    ap.add_argument("--merges", default=None)
    ap.add_argument("--vocab", default=None)
    ap.add_argument("--captions", type=int, default=200000)
    ap.add_argument("--reports", type=int, default=20000)
    ap.add_argument("--host_rows", type=int, default=20000)
    ap.add_argument("--tower_rows", type=int, default=20000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--passes", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tokenize_time: no GPU (a timing needs one; there is no fallback)")
    from lemon_amd import tokenizer as tk
    from lemon_amd.biomed import BiomedCLIP, BiomedConfig
    from lemon_amd.clip import ClipConfig, LemonCLIP
    from lemon_amd.pipeline import Embedder
    dev = torch.device("cuda")
    words, ranks = words_and_merges()
    bpe = tk.ClipBPE.from_file(args.merges) if args.merges else tk.ClipBPE(ranks)
    bert = tk.BertWordPiece.from_file(args.vocab, 256) if args.vocab else tk.BertWordPiece(piece_vocab(words), 256)
    jobs = [("clip", tk.ClipTokenize(bpe, 77), make_corpus(words, args.captions, 6, 40, 1), args.host_rows, args.tower_rows,
             lambda: LemonCLIP(ClipConfig.named("vit-b-32"))),
            ("bert", bert, make_corpus(words, args.reports, 150, 200, 2), max(1, args.host_rows // 10), max(1, args.tower_rows // 4),
             lambda: BiomedCLIP(BiomedConfig()))]
    res = {"device": torch.cuda.get_device_name(0), "passes": args.passes, "batch": args.batch, "merges": args.merges or "fixture (sparse)",
           "vocab": args.vocab or "pieces of the corpus words", "corpora": {}}
    for name, host, texts, host_rows, tower_rows, make_model in jobs:
        on_device = tk.device_form(host, dev)
        if on_device is None:
            raise SystemExit(f"tokenize_time: {name} has no device form here (ftfy installed, or the vocabulary does not fit)")
        sample = texts[:host_rows]
        want = host(sample)
        got = on_device(sample)
        if not torch.equal(got.cpu(), want):
            raise SystemExit(f"tokenize_time: {name}: device ids differ from the host's")
        lengths = on_device.lengths.numpy()
        t_host = timed(lambda: host(sample), args.passes, lambda: None)

        def device_pass():
            declined = 0
            for s in range(0, len(texts), args.batch):
                on_device(texts[s:s + args.batch])
                declined += on_device.declined
            return declined

        declined = device_pass()
        t_dev = timed(device_pass, args.passes, torch.cuda.synchronize)
        emb = Embedder(make_model(), dev, text_dedup=False)
        ids = torch.cat([on_device(texts[s:s + args.batch]) for s in range(0, tower_rows, args.batch)])[:tower_rows]
        t_tower = timed(lambda: emb.embed_texts(ids), args.passes, torch.cuda.synchronize)
        emb.raise_if_nonfinite()
        del emb
        torch.cuda.empty_cache()
        rate = lambda rows, ts: round(rows / sorted(ts)[len(ts) // 2], 1)
        res["corpora"][name] = {
            "rows": len(texts), "bytes": sum(map(len, texts)), "context": on_device.ctx, "declined_rows": declined,
            "tokens_per_row": {"min": int(lengths.min()), "mean": round(float(lengths.mean()), 1), "max": int(lengths.max())},
            "host": {"rows": len(sample), "seconds": [round(t, 4) for t in t_host], "captions_per_s": rate(len(sample), t_host)},
            "device": {"rows": len(texts), "seconds": [round(t, 4) for t in t_dev], "captions_per_s": rate(len(texts), t_dev)},
            "tower": {"rows": int(ids.shape[0]), "seconds": [round(t, 4) for t in t_tower], "captions_per_s": rate(int(ids.shape[0]), t_tower)}}
        print(name, json.dumps(res["corpora"][name]), flush=True)
    out = args.out if os.path.isabs(args.out) else os.path.join(ROOT, args.out)
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "tokenize_time.json"), "w") as fh:
        json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
