"""CPU: ops.block_plan -- which path serves each part of a transformer block -- against recorded decisions.

tests/golden/block_plan.txt was NOT written by block_plan: a stand-alone script holding the predicates of clip.Block.forward,
Block._forward_split, Block.forward_chain and biomed.BertLayer.chain_supported as they stood at commit a37fab2 (the parent of
the commit that introduced the plan; library calls replaced by the names of the paths, the head-dim mode and the width cap
arguments) wrote it.  That script and block_plan agreed on the whole product of W in {48, 256, 512, 768, 1024, 1280, 2048, 2304},
mlp in {4 W, 4 W + 32}, head counts giving head dims 64 and 80 plus 7 (divides no W), L in {8, 77, 288, 289, 577, 4096, 4097},
pooled, carry, the three GEMM modes, the three MLP modes, the fold, the three chain levels, the head-dim mode, the width caps
1024 and fused_width_max(), fused and not; the committed subset keeps every 211th row of it and two rows of every distinct
decision per width, GEMM mode and cap."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "block_plan.txt")
INPUTS = ("fused", "width", "mlp", "heads", "seq_len", "pooled", "carry", "gemm_mode", "mlp_mode", "ln_fold", "chain_res", "head_dims", "width_cap")
TEXT = ("gemm_mode", "mlp_mode")


def table_rows():
    rows = []
    for ln in open(TABLE):
        if ln.strip() and not ln.startswith("#"):
            case, row = ln.strip().split(" | ")
            args = {f: (v if f in TEXT else int(v)) for f, v in zip(INPUTS, case.split())}
            qkv, attn, out, mlp, chain, lean = row.split()
            rows.append((args, dict(qkv=qkv, attn=attn, out=out, mlp=mlp, chain=bool(int(chain)), lean=int(lean))))
    return rows


def test_the_plan_reproduces_every_recorded_decision():
    from lemon_amd import ops
    rows = table_rows()
    assert len(rows) >= 1000
    for args, want in rows:
        p = ops.block_plan(**args)
        got = dict(qkv=p.qkv, attn=p.attn, out=p.out, mlp=p.mlp, chain=p.chain, lean=p.lean)
        assert got == want and p.mode == args["gemm_mode"], (args, got, want)


def test_the_table_covers_what_it_has_to():
    rows = table_rows()
    seen = {f: {a[f] for a, _ in rows} for f in INPUTS}
    assert seen["width"] == {48, 256, 512, 768, 1024, 1280, 2048, 2304} and seen["seq_len"] == {8, 77, 288, 289, 577, 4096, 4097}
    assert seen["gemm_mode"] == {"f32", "bf16x6", "f16x3"} and seen["mlp_mode"] == {"lib", "fused", "block"}
    assert seen["chain_res"] == {0, 1, 2} and seen["width_cap"] == {1024, 2048}
    for f in ("fused", "pooled", "carry", "ln_fold", "head_dims"):
        assert seen[f] == {0, 1}, f
    assert any(a["mlp"] % 256 for a, _ in rows) and any(a["width"] % a["heads"] for a, _ in rows)
    assert {a["width"] // a["heads"] for a, _ in rows if a["width"] % a["heads"] == 0} >= {64, 80}
    for field, values in (("qkv", {"torch", "f32", "split", "tiled", "tiled_ln"}), ("attn", {"sdpa", "f32", "split", "tiled"}),
                          ("out", {"torch", "f32", "split", "tiled"}), ("mlp", {"torch", "f32", "split", "tiled"}), ("lean", {0, 1, 2})):
        assert {w[field] for _, w in rows} == values, field
    # the chain at every lean level, under both caps; the width between the caps chains under the wider one only
    assert {(a["width_cap"], w["lean"]) for a, w in rows if w["chain"]} == {(c, r) for c in (1024, 2048) for r in (0, 1, 2)}
    assert any(w["chain"] and a["width"] == 1280 and a["width_cap"] == 2048 for a, w in rows)
    assert any(not w["chain"] and w["qkv"] == "f32" and a["width"] == 1280 and a["width_cap"] == 1024 and a["head_dims"] == 1
               and a["gemm_mode"] == "f16x3" for a, w in rows)
    # the pooled block behind a chain folds the LayerNorm into its QKV GEMM and runs the rest in the library
    assert any(a["pooled"] and a["carry"] and (w["qkv"], w["attn"], w["out"], w["mlp"]) == ("tiled_ln", "f32", "split", "split") for a, w in rows)


def test_the_plan_is_pure():
    import inspect
    from lemon_amd import ops
    src = inspect.getsource(ops.block_plan) + inspect.getsource(ops._attention_takes) + inspect.getsource(ops.mlp_fused_supported)
    for word in ("torch.", "import", "environ", "_lib", "attention_head_dims", "gemm_mode()", "mlp_mode()"):
        assert word not in src, word
