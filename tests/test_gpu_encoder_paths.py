"""GPU: which library entries the encoder towers call, in which order and with which arguments, under every knob row of the
block plan (ops.block_plan) -- against traces recorded before the plan existed.

A recording proxy stands in for lemon_amd._lib._lib (monkeypatch): it logs every lemon_* call as "name(args)" -- integers and
floats as they are, pointers as p / 0 (null) -- and forwards it.  The towers are the smallest on which the hand-written paths
still engage (width 256, 4 heads, mlp 256, three layers: a chain head without carry, a chained block with carry, the pooled last
block) plus the `tiny` architecture (widths 48 and 40: the fallbacks).

tests/golden/encoder_call_traces.json was recorded with THIS recorder (`python tests/test_gpu_encoder_paths.py OUT.json` with
the package of commit a37fab2 -- the parent of the commit that introduced ops.block_plan -- first on the module path) on an
MI355X.  It holds entry names, shapes, knob-derived integers, null masks and the GEMMs' alpha / LayerNorm eps (powers of two and
constants of the seeded CPU initialisation): nothing a kernel computed.  Not traced: lemon_linear_f16x3t_last_kernel (it did not
exist then), the once-per-process calls (tuned-solution loading, error text), and lemon_attention_get_head_dims -- a getter
without side effects, which the hand-written predicates asked between zero and two times per block depending on where an `and`
stopped and the plan asks once; its calls were dropped from the recording.  Every call that launches or sets something is
compared, lemon_attention_set_f16 included."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "encoder_call_traces.json")
NOT_TRACED = ("lemon_linear_f16x3t_last_kernel", "lemon_linear_load_tuned", "lemon_last_error", "lemon_attention_get_head_dims")

# knob rows: (name, environment, forced GEMM mode or None, forced LayerNorm fold or None)
_F16 = dict(LEMON_GEMM="f16x3")
KNOBS = [
    ("f32", dict(LEMON_GEMM="f32"), None, None),
    ("bf16x6", dict(LEMON_GEMM="bf16x6"), None, None),
    ("f16x3-lib", dict(_F16, LEMON_MLP="lib"), None, None),
    ("f16x3-fused", dict(_F16, LEMON_MLP="fused"), None, None),
    ("f16x3-block-nofold", dict(_F16, LEMON_MLP="block", LEMON_LNFOLD="0"), None, None),
    ("f16x3-block-fold-res0", dict(_F16, LEMON_MLP="block", LEMON_LNFOLD="1", LEMON_CHAIN_RES="0"), None, None),
    ("f16x3-block-fold-res1", dict(_F16, LEMON_MLP="block", LEMON_LNFOLD="1", LEMON_CHAIN_RES="1"), None, None),
    ("f16x3-block-fold-res2", dict(_F16, LEMON_MLP="block", LEMON_LNFOLD="1", LEMON_CHAIN_RES="2"), None, None),
    ("forced-bf16x6", {}, "bf16x6", None),
    ("forced-nofold", {}, None, False),
]
KNOB_VARS = ("LEMON_GEMM", "LEMON_MLP", "LEMON_LNFOLD", "LEMON_CHAIN_RES", "LEMON_ATTN_F16", "LEMON_ATTN_HEAD_DIMS", "LEMON_BERT_BUCKET")


class _Recorder:
    """stands in for the loaded library: logs every lemon_* call, then makes it"""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("lemon_") or name in NOT_TRACED:
            return fn

        def call(*args):
            self._log.append(f"{name}({','.join(_arg(a) for a in args)})")
            return fn(*args)
        return call


def _arg(a):
    if isinstance(a, bool):
        return str(int(a))
    if isinstance(a, int):
        return str(a)
    if isinstance(a, float):
        return repr(a)
    if a is None or getattr(a, "value", 1) is None:            # None, c_void_p(0)
        return "0"
    return "p"


def _towers():
    """{name: run()} -- seeded CPU initialisation and inputs, so that the weights' power-of-two scales are the same everywhere"""
    from lemon_amd.biomed import BiomedCLIP, BiomedConfig
    from lemon_amd.clip import ClipConfig, LemonCLIP, TowerConfig
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(5)
    small = TowerConfig(256, 3, 4, 256)
    clip = LemonCLIP(ClipConfig(embed_dim=32, image_size=32, patch_size=8, vision=small, text=small, vocab_size=300, context_length=16,
                                eos_token_id=299)).to(dev).eval()
    tiny = LemonCLIP(ClipConfig.named("tiny")).to(dev).eval()
    bio = BiomedCLIP(BiomedConfig(embed_dim=32, image_size=32, patch_size=8, vision=small, text=small, vocab_size=300, context_length=16,
                                  max_positions=32, proj_hidden=48)).to(dev).eval()
    pixels = torch.randn(2, 3, 32, 32, generator=g).to(dev)

    def ids(counts, last, first=None):
        t = torch.zeros(len(counts), 16, dtype=torch.long)
        for i, c in enumerate(counts):
            t[i, :c] = torch.randint(4, 290, (c,), generator=g)
            if first is not None:
                t[i, 0] = first
            t[i, c - 1] = last
        return t.to(dev)

    clip_ids = ids((6, 10, 13), 299)                            # ragged EOT positions: 16 tokens run
    bert_ids = ids((16, 11, 9), 3, first=2)                      # [CLS] ... [SEP], pads behind
    bert_full = ids((16, 16, 16), 3, first=2)

    def bucketed(tower, n):
        def run():
            prev, tower.length_bucket = tower.length_bucket, n
            try:
                return tower(bert_ids, lengths=[16, 11, 9]) if n else tower(bert_full)
            finally:
                tower.length_bucket = prev
        return run

    models = (clip, tiny, bio)
    return models, {
        "clip_vision": lambda: clip.vision(pixels),
        "clip_text": lambda: clip.text(clip_ids),
        "biomed_vision": lambda: bio.vision(pixels),
        "biomed_text_lengths": bucketed(bio.text, 8),
        "biomed_text_exact": bucketed(bio.text, 0),
        "tiny_vision": lambda: tiny.vision(pixels),
        "tiny_text": lambda: tiny.text(clip_ids),
    }


def trace_row(mp, knob, models, towers):
    """{tower: [calls]} of one knob row; mp: a pytest MonkeyPatch"""
    from lemon_amd import _lib, ops
    name, env, gemm, fold = knob
    for v in KNOB_VARS:
        mp.delenv(v, raising=False)
    for k, v in env.items():
        mp.setenv(k, v)
    out = {}
    for tname, run in towers.items():
        for model in models:                                   # packed / split weights are made again in every row
            for mod in model.modules():
                mod.__dict__.pop("_split_cache", None)
        log = []
        with pytest.MonkeyPatch.context() as swap, torch.no_grad():
            swap.setattr(_lib, "_lib", _Recorder(_lib.load(), log))
            if gemm is not None:
                with ops.gemm_mode_forced(gemm):
                    y = run()
            elif fold is not None:
                with ops.ln_fold_forced(fold):
                    y = run()
            else:
                y = run()
            torch.cuda.synchronize()
        assert bool(torch.isfinite(y).all()), (name, tname)
        out[tname] = log
    return out


@pytest.fixture(scope="module")
def towers(hip):
    return _towers()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    return {key: g["traces"][i] for key, i in g["rows"].items()}


@pytest.mark.parametrize("knob", KNOBS, ids=[k[0] for k in KNOBS])
def test_call_trace_equals_the_recorded_one(towers, golden, knob):
    models, runs = towers
    with pytest.MonkeyPatch.context() as mp:
        got = trace_row(mp, knob, models, runs)
    for tname, log in got.items():
        want = golden[f"{knob[0]}/{tname}"]
        assert len(log) > 10 and all(c.startswith("lemon_") for c in log)
        for i, (a, b) in enumerate(zip(log, want)):
            assert a == b, f"{knob[0]}/{tname}: call {i} is {a}, recorded {b}"
        assert len(log) == len(want), f"{knob[0]}/{tname}: {len(log)} calls, recorded {len(want)}"


def test_the_traces_reach_every_path(golden):
    assert set(golden) == {f"{k[0]}/{t}" for k in KNOBS for t in ("clip_vision", "clip_text", "biomed_vision", "biomed_text_lengths",
                                                               "biomed_text_exact", "tiny_vision", "tiny_text")}
    names = lambda key: {c.split("(")[0] for c in golden[key]}
    full = names("f16x3-block-fold-res2/clip_vision")
    assert {"lemon_rowstats_f16x3t", "lemon_linear_f16x3t_ln", "lemon_linear_f16x3t_chain", "lemon_ln_finalize", "lemon_attention_f16x3t"} <= full
    assert "lemon_linear_f16x3t_chain" not in names("f16x3-block-nofold/clip_vision") and "lemon_linear_f16x3t" in names("f16x3-block-nofold/clip_vision")
    assert "lemon_linear_f16x3t" in names("f16x3-fused/clip_text") and "lemon_linear_f16x3" in names("f16x3-fused/clip_text")
    assert "lemon_linear_f16x3t" not in names("f16x3-lib/clip_text")
    assert "lemon_linear_bf16x6" in names("forced-bf16x6/clip_text") and "lemon_linear_f32" in names("f32/clip_text")
    assert "lemon_attention_f16x3t_varlen" in names("f16x3-block-fold-res2/biomed_text_lengths")
    assert "lemon_linear_f16x3t" not in names("f16x3-block-fold-res2/tiny_vision")          # widths 48 / 40: no hand-written GEMM
    # the three lean levels of the residual stream differ, and so do the fold and its fallback
    res = [golden[f"f16x3-block-fold-res{i}/clip_vision"] for i in (0, 1, 2)]
    assert res[0] != res[1] != res[2] != res[0]
    assert golden["forced-nofold/clip_vision"] == golden["f16x3-block-nofold/clip_vision"]


if __name__ == "__main__":
    # the recorder: python tests/test_gpu_encoder_paths.py OUT.json, with the package to record first on the module path
    models_, runs_ = _towers()
    traces, rows = [], {}
    with pytest.MonkeyPatch.context() as mp_:
        for knob_ in KNOBS:
            for tname_, log_ in trace_row(mp_, knob_, models_, runs_).items():
                if log_ not in traces:
                    traces.append(log_)
                rows[f"{knob_[0]}/{tname_}"] = traces.index(log_)
    with open(sys.argv[1], "w") as f_:
        json.dump({"traces": traces, "rows": rows}, f_, indent=0)
    print(f"{len(rows)} rows, {len(traces)} distinct traces, {sum(map(len, traces))} calls")
