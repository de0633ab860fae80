"""Time the streaming attention kernels (seq_len > 288) next to what ran for these shapes before them, the SDPA expression of
clip.Block._sdpa on the same qkv in the same process:  python tools/attn_long_time.py [--out profiles/attention_long/attn_long.json]

Per shape (B, L, H, causal): device-event time of the fp32 output (ops.attention) and of the tile-major operand output
(ops.attention_t) in both arithmetic forms (lemon_attention_set_f16 1 / 0), and of
    view / permute -> F.scaled_dot_product_attention (fp32) -> transpose / reshape,
alternating, three draws of 20 launches each; every draw is written out.  TB/s by the byte model of csrc/attention.hip's header:
16 * H * 64 bytes per token (three reads, one write)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from lemon_amd import _lib, ops

SHAPES = ((64, 577, 16, False), (128, 577, 12, False), (32, 1025, 12, False), (64, 512, 8, True))
DRAWS, REPS = 3, 20


def sdpa(qkv, H, causal):
    B, L, W3 = qkv.shape
    W = W3 // 3
    q, k, v = qkv.view(B, L, 3, H, W // H).permute(2, 0, 3, 1, 4)
    return F.scaled_dot_product_attention(q, k, v, is_causal=causal).transpose(1, 2).reshape(B, L, W)


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3          # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "attention_long", "attn_long.json"))
    args = ap.parse_args()
    lib = _lib.load()
    records = []
    for B, L, H, causal in SHAPES:
        qkv = torch.randn(B, L, 3 * H * 64, device="cuda")
        runs = [("stream_f16/f32out", 1, lambda: ops.attention(qkv, H, causal)), ("stream_f16/tiled", 1, lambda: ops.attention_t(qkv, H, causal)),
                ("stream_f32/f32out", 0, lambda: ops.attention(qkv, H, causal)), ("stream_f32/tiled", 0, lambda: ops.attention_t(qkv, H, causal)),
                ("sdpa", None, lambda: sdpa(qkv, H, causal))]
        us = {name: [] for name, _, _ in runs}
        prev = lib.lemon_attention_set_f16(1)
        try:
            for _ in range(DRAWS):
                for name, f16, fn in runs:
                    if f16 is not None:
                        lib.lemon_attention_set_f16(f16)
                    us[name].append(timed(fn))
        finally:
            lib.lemon_attention_set_f16(prev)
        gb = B * L * H * 64 * 16 / 1e9
        rec = {"batch": B, "seq_len": L, "heads": H, "causal": causal, "model_gbytes": gb, "draws": DRAWS, "launches_per_draw": REPS,
               "us": us, "tb_per_s": {n: [gb / (t * 1e-6) / 1e3 for t in v] for n, v in us.items() if n != "sdpa"},
               "sdpa_over_stream": {n: [s / t for s, t in zip(us["sdpa"], v)] for n, v in us.items() if n != "sdpa"},
               "slowest_stream_over_fastest_sdpa": {n: max(v) / min(us["sdpa"]) for n, v in us.items() if n != "sdpa"}}
        records.append(rec)
        print(f"B={B} L={L} H={H} causal={causal}: " + "  ".join(
            f"{n} {min(v):.1f}-{max(v):.1f} us" + ("" if n == "sdpa" else f" ({gb / (min(v) * 1e-6) / 1e3:.2f} TB/s)") for n, v in us.items()), flush=True)
        del qkv
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "shapes": records}, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
