"""Time attention at head dims beyond 64 (csrc/attention_hd.hip, lemon_attention_set_head_dims) next to what runs for these
towers with the switch off, the SDPA expression of clip.Block._sdpa on the same qkv in the same process:

    python tools/attn_hd_time.py [--out profiles/attention_hd/attn_hd.json]
    python tools/attn_hd_time.py --tower [--batch 32] [--draws 3] [--out profiles/attention_hd/encode_vit-h-14.json]

Kernel level, per shape (B, L, H, head_dim): device-event time of the fp32 output (ops.attention) and of the tile-major operand
output (ops.attention_t) of k_attention_hdx_stream and of
    view / permute -> F.scaled_dot_product_attention (fp32) -> transpose / reshape,
alternating, three draws of 20 launches each; every draw is written out.  At head_dim 64 additionally the shipped
fp32-arithmetic kernel (mode 0) against the new one (mode 2).  TB/s by the byte model of csrc/attention.hip's header:
16 * H * head_dim bytes per token (three reads, one write).

Tower level (--tower): encode_image of a full-size ViT-H/14 (ClipConfig.named('vit-h-14'), random weights, default GEMM mode),
images/s with LEMON_ATTN_HEAD_DIMS=1 against 0, one FRESH process per draw (2 warm-up + 5 timed batches), alternating.  The
rule for flipping the default: on is not slower than off beyond the spread of the draws."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((64, 257, 16, 80), (64, 257, 16, 104), (32, 577, 16, 80), (64, 257, 16, 128))
SHAPES_64 = ((64, 257, 16), (64, 577, 16))
DRAWS, REPS = 3, 20


def sdpa(qkv, H):
    import torch.nn.functional as F
    B, L, W3 = qkv.shape
    W = W3 // 3
    q, k, v = qkv.view(B, L, 3, H, W // H).permute(2, 0, 3, 1, 4)
    return F.scaled_dot_product_attention(q, k, v, is_causal=False).transpose(1, 2).reshape(B, L, W)


def timed(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS * 1e3          # us


def kernel_level(out):
    import torch
    from lemon_amd import _lib, ops
    lib = _lib.load()
    records = []
    prev_mode, prev_f16 = ops.set_attention_head_dims(1), lib.lemon_attention_set_f16(0)
    try:
        for B, L, H, hd in SHAPES:
            qkv = torch.randn(B, L, 3 * H * hd, device="cuda")
            runs = [("hdx/f32out", lambda: ops.attention(qkv, H)), ("hdx/tiled", lambda: ops.attention_t(qkv, H)), ("sdpa", lambda: sdpa(qkv, H))]
            us = {name: [] for name, _ in runs}
            for _ in range(DRAWS):
                for name, fn in runs:
                    us[name].append(timed(fn))
            gb = B * L * H * hd * 16 / 1e9
            records.append({"batch": B, "seq_len": L, "heads": H, "head_dim": hd, "model_gbytes": gb, "draws": DRAWS, "launches_per_draw": REPS,
                            "us": us, "tb_per_s": {n: [gb / (t * 1e-6) / 1e3 for t in v] for n, v in us.items() if n != "sdpa"},
                            "sdpa_over_hdx": {n: [s / t for s, t in zip(us["sdpa"], v)] for n, v in us.items() if n != "sdpa"}})
            print(f"B={B} L={L} H={H} hd={hd}: " + "  ".join(f"{n} {min(v):.1f}-{max(v):.1f} us" for n, v in us.items()), flush=True)
            del qkv
            torch.cuda.empty_cache()
        for B, L, H in SHAPES_64:       # the new kernel on the shipped kernel's ground (fp32 arithmetic in both)
            qkv = torch.randn(B, L, 3 * H * 64, device="cuda")
            us = {"shipped_f32/tiled": [], "hdx/tiled": []}
            for _ in range(DRAWS):
                for name, mode in (("shipped_f32/tiled", 0), ("hdx/tiled", 2)):
                    ops.set_attention_head_dims(mode)
                    us[name].append(timed(lambda: ops.attention_t(qkv, H)))
            records.append({"batch": B, "seq_len": L, "heads": H, "head_dim": 64, "draws": DRAWS, "launches_per_draw": REPS, "us": us})
            print(f"B={B} L={L} H={H} hd=64: " + "  ".join(f"{n} {min(v):.1f}-{max(v):.1f} us" for n, v in us.items()), flush=True)
    finally:
        ops.set_attention_head_dims(prev_mode)
        lib.lemon_attention_set_f16(prev_f16)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "shapes": records}, f, indent=1)
    print("wrote", out)


def tower_draw(batch):
    """one draw in this (fresh) process: prints a JSON line"""
    import torch
    from lemon_amd import ops
    from lemon_amd.clip import ClipConfig, LemonCLIP
    cfg = ClipConfig.named("vit-h-14")
    model = LemonCLIP(cfg).eval().cuda()
    px = torch.randn(batch, 3, cfg.image_size, cfg.image_size, device="cuda")
    for _ in range(2):
        y = model.encode_image(px)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        y = model.encode_image(px)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / 5
    print(json.dumps({"head_dims_mode": ops.attention_head_dims(), "ms_per_batch": round(ms, 3), "images_per_s": round(batch / ms * 1e3, 1),
                      "finite": bool(torch.isfinite(y).all()), "device": torch.cuda.get_device_name(0)}), flush=True)


def tower_level(out, batch, draws):
    res = {"on": [], "off": []}
    device = None
    for _ in range(draws):
        for name, mode in (("on", "1"), ("off", "0")):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--tower-draw", "--batch", str(batch)], cwd=ROOT,
                               env=dict(os.environ, LEMON_ATTN_HEAD_DIMS=mode), capture_output=True, text=True, timeout=900)
            if r.returncode != 0:
                raise RuntimeError(f"tower draw ({name}) failed with {r.returncode}: {r.stderr[-2000:]}")
            rec = json.loads(r.stdout.strip().splitlines()[-1])
            assert rec["head_dims_mode"] == int(mode) and rec["finite"], rec
            device = rec.pop("device")
            res[name].append(rec)
            print(name, rec, flush=True)
    doc = {"what": f"encode_image of a full-size ViT-H/14 (257 tokens, head_dim 80, random weights, batch {batch}, default GEMM mode), "
                   "images/s with LEMON_ATTN_HEAD_DIMS=1 against 0, alternating, one fresh process per draw (2 warm-up + 5 timed batches)",
           "device": device, "draws": res,
           "factor_per_draw": [round(a["images_per_s"] / b["images_per_s"], 3) for a, b in zip(res["on"], res["off"])]}
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
    print("wrote", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--tower", action="store_true")
    ap.add_argument("--tower-draw", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--draws", type=int, default=DRAWS)
    args = ap.parse_args()
    if args.tower_draw:
        tower_draw(args.batch)
    elif args.tower:
        tower_level(args.out or os.path.join("profiles", "attention_hd", "encode_vit-h-14.json"), args.batch, args.draws)
    else:
        kernel_level(args.out or os.path.join("profiles", "attention_hd", "attn_hd.json"))


if __name__ == "__main__":
    main()
