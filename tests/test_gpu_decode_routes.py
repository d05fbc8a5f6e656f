"""The decode step's route and launches, pinned: for a dozen (model, batch, cache, ZL_* switch, entry point) cases the ordered zl_* symbols
one step calls, recorded at the commit BEFORE LLaMA.encode was given one route decision and one layer body (tests/golden/
decode_step_calls.json, "calls"), and the four strings of the _DecodeRoute the step decides ("route").  A change that adds, drops or
reorders a launch of the decode step, or sends a case down another route, fails here by name.

"queries" are the route decision's host-only questions to the library (workspace sizes, split lengths, whether a launcher takes /
leaves the rows' statistics): they launch nothing, and they are kept in a list of their own because the decision sits in front of
the step's first launch now and sat behind it when the lists were recorded.

To regenerate (after a deliberate change of the step's launches): `python tests/test_gpu_decode_routes.py` on the GPU rewrites the
call lists and the routes from the checked-out code (with the argument `routes`: the routes only, the call lists stay); review the
diff of the JSON file like code."""
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_step_calls.json")
QUERIES = {"zl_decode_attn_workspace_bytes", "zl_decode_attn_split_len", "zl_device_cu_count", "zl_decode_attn_la_split_len",
           "zl_decode_attn_la_workspace_bytes", "zl_w4a16_emits_row_ss", "zl_w4a16_takes_row_ss", "zl_w4a16_scratch_bytes"}
SWITCHES = ("ZL_ATTN_MFMA", "ZL_FUSE_QKV_ROPE", "ZL_ATTN_MERGE", "ZL_ATTN_MERGE_MAX_B", "ZL_ATTN_LA", "ZL_ATTN_LA_SPLIT", "ZL_ATTN_LA_HALF",
            "ZL_ROW_SS", "ZL_ROW_SS_MIN_M", "ZL_DEFER_NORM", "ZL_W4_SMALL_ALGO", "ZL_FUSE_O_GATEUP", "ZL_W8_PHASE", "KV_CACHE_DTYPE")
# name: (model, batch, INT8 KV cache, environment, entry point)
CASES = {
    "gptq b1": ("gptq", 1, False, {}, "encode"),
    "gptq b3": ("gptq", 3, False, {}, "encode"),
    "gptq b9": ("gptq", 9, False, {}, "encode"),
    "gptq b32": ("gptq", 32, False, {}, "encode"),
    "gptq b3 ZL_ATTN_LA=0": ("gptq", 3, False, {"ZL_ATTN_LA": "0"}, "encode"),
    "gptq b1 ZL_ATTN_MERGE=0": ("gptq", 1, False, {"ZL_ATTN_MERGE": "0"}, "encode"),
    "gptq b3 ZL_FUSE_QKV_ROPE=0": ("gptq", 3, False, {"ZL_FUSE_QKV_ROPE": "0"}, "encode"),
    "gptq b3 ZL_ATTN_MFMA=0": ("gptq", 3, False, {"ZL_ATTN_MFMA": "0"}, "encode"),
    "gptq b3 int8 kv": ("gptq", 3, True, {}, "encode"),
    "wide b9": ("wide", 9, False, {}, "encode"),
    "wide b9 ZL_ROW_SS=0": ("wide", 9, False, {"ZL_ROW_SS": "0"}, "encode"),
    "wide b4 verify causal": ("wide", 4, False, {}, "verify_causal"),
    "int8 b3": ("int8", 3, False, {}, "encode"),
    "head64 b1": ("head64", 1, False, {}, "encode"),
    "gptq b1 verify causal": ("gptq", 1, False, {}, "verify_causal"),
    "gptq b1 verify rows": ("gptq", 1, False, {}, "verify_rows"),
}
_MODELS = {}


class _Recorder:
    """stands where ops.lib() returns the C library: notes the name of every zl_* symbol called, in order"""

    def __init__(self, real):
        self._real, self.calls, self.queries = real, [], []

    def __getattr__(self, name):
        f = getattr(self._real, name)
        if not name.startswith("zl_"):
            return f

        def call(*args):
            (self.queries if name in QUERIES else self.calls).append(name)
            return f(*args)
        return call


def _model(kind, dev):
    from test_gpu_model import _dense_state, _hf_state
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    if kind not in _MODELS:
        cfg = ModelConfig(num_layers=2, dim_model=1024, num_heads=8, dim_head=128, dim_ff=2048, vocab_size=512, num_kv_heads=2, eps=1e-5,
                          rope_theta=5e5)
        if kind == "gptq":
            sd = _hf_state(np.random.default_rng(0), cfg, 128)
            m = LLaMA(cfg, QuantConfig(5, 128), dev).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        elif kind == "int8":
            sd = _dense_state(np.random.default_rng(23), cfg)
            m = LLaMA(cfg, QuantConfig(2, 0), dev).load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        elif kind == "wide":                               # Llama-3-8B's layer geometry, where the rows' statistics route applies
            cfg = ModelConfig.llama3_8b()
            cfg.num_layers, cfg.vocab_size = 2, 512
            m = LLaMA(cfg, QuantConfig(5, 128), dev).init_synthetic(seed=5)
        else:                                              # MiniCPM's geometry (bf16, head size 64) with 2 layers and a small vocabulary
            cfg = ModelConfig.minicpm_2b()
            cfg.num_layers, cfg.vocab_size = 2, 1024
            m = LLaMA(cfg, QuantConfig(0, 0), dev).init_random(seed=3)
        _MODELS[kind] = m
    return _MODELS[kind]


def _second_step(setattr_, dev, kind, batch, kv_int8, env, entry):
    """(calls, queries, route) of the second of two consecutive steps: the first allocates the per-batch workspaces and packs what is
    packed on first use.  setattr_(object, name, value): monkeypatch.setattr, or plain setattr when regenerating"""
    from zhilight_amd import _lib, llama, ops
    real, decide = ops.lib, getattr(llama.LLaMA, "_decode_route", None)
    rec, routes = _Recorder(_lib.lib()), []

    def spy(self, *a, **kw):
        routes.append(decide(self, *a, **kw))
        return routes[-1]
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    try:
        os.environ.update(env)
        model = _model(kind, dev)
        torch.manual_seed(7)
        ctx = model.new_context(batch, 128, 40, fill_random=True, kv_cache_dtype="int8" if kv_int8 else None)
        ctx.tokens.copy_(torch.randint(0, model.cfg.vocab_size, (batch,), device=dev, dtype=torch.int32))
        drafts = torch.randint(0, model.cfg.vocab_size, (batch, 3), device=dev, dtype=torch.int32)
        step = {"encode": lambda: model.encode(ctx), "gemv_only": lambda: model.encode(ctx, gemv_only=True),
                "step_greedy": lambda: model.step_greedy(ctx), "skip_gemv": lambda: model.step_greedy(ctx, skip_gemv=True),
                "verify_causal": lambda: model.verify(ctx, drafts, attn="causal"), "verify_rows": lambda: model.verify(ctx, drafts, attn="rows")}[entry]
        step()
        if decide is not None:
            setattr_(llama.LLaMA, "_decode_route", spy)
        for mod in (ops, _lib):                            # every module that binds lib
            setattr_(mod, "lib", lambda: rec)
        step()
        torch.cuda.synchronize()
    finally:
        for mod in (ops, _lib):
            setattr_(mod, "lib", real)
        if decide is not None:
            setattr_(llama.LLaMA, "_decode_route", decide)
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update({k: v for k, v in saved.items() if v is not None})
    route = {f: getattr(routes[0], f) for f in ("qkv", "norm", "attn", "out")} if routes else None
    return rec.calls, rec.queries, route


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        yield json.load(f)
    _MODELS.clear()                                        # the models leave the GPU with the module


@pytest.mark.parametrize("case", list(CASES))
def test_decode_step_calls_and_route(dev, monkeypatch, golden, case):
    """one step's zl_* symbols, in order, are the recorded ones, and so are the route's four strings"""
    calls, queries, route = _second_step(monkeypatch.setattr, dev, *CASES[case])
    assert route == golden[case]["route"]
    assert calls == golden[case]["calls"]
    assert queries == golden[case]["queries"]


ATTENTION = {"zl_decode_attn", "zl_decode_attn_ex", "zl_decode_attn_la", "zl_decode_attn_splits", "zl_decode_attn_fused", "zl_decode_attn_quant",
             "zl_decode_attn_quant_ex", "zl_decode_attn_causal"}
EMBED_ROPE = {"zl_embedding", "zl_embedding_rope", "zl_rope_cos_sin", "zl_rope_cos_sin_llama3"}
LM_HEAD = {"zl_gemm_nt_small_m", "zl_gemm_nt_small_m_argmax", "zl_gemm_nt", "zl_gemm_nt_packed"}


@pytest.mark.parametrize("kind", ["gptq", "int8"])
def test_bench_legs_split_the_step(dev, monkeypatch, kind):
    """bench.py's two legs at 3 rows.  W4 route: encode(gemv_only=True) is the full step minus its attention, embedding / rope-table and
    lm_head launches (it makes its rope table with a launch of its own, not counted), step_greedy(skip_gemv=True) the full greedy
    step minus exactly those projections.  W8 route: the legs are not wired in -- gemv_only runs the whole layers (attention
    included) and only drops the embedding and the lm_head, skip_gemv runs the whole step."""
    full = _second_step(monkeypatch.setattr, dev, kind, 3, False, {}, "encode")[0]
    gemv = [s for s in _second_step(monkeypatch.setattr, dev, kind, 3, False, {}, "gemv_only")[0] if s not in EMBED_ROPE]
    greedy = _second_step(monkeypatch.setattr, dev, kind, 3, False, {}, "step_greedy")[0]
    skip = _second_step(monkeypatch.setattr, dev, kind, 3, False, {}, "skip_gemv")[0]
    assert any(s in ATTENTION for s in full) and any(s in LM_HEAD for s in full) and any(s in EMBED_ROPE for s in full)
    if kind == "gptq":
        assert gemv == [s for s in full if s not in ATTENTION | EMBED_ROPE | LM_HEAD] and gemv
        assert not set(gemv) & set(skip)
        assert skip == [s for s in greedy if s not in set(gemv)]
    else:
        assert gemv == [s for s in full if s not in EMBED_ROPE | LM_HEAD]
        assert skip == greedy


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    old = json.load(open(GOLDEN)) if os.path.exists(GOLDEN) else {}
    new = {}
    for name, case in CASES.items():
        calls, queries, route = _second_step(setattr, torch.device("cuda:0"), *case)
        if sys.argv[1:] == ["routes"]:
            calls, queries = old[name]["calls"], old[name]["queries"]
        new[name] = {"route": route if route is not None else old.get(name, {}).get("route"), "calls": calls, "queries": queries}
        print(name, new[name]["route"], len(calls), "calls")
    with open(GOLDEN, "w") as f:
        json.dump(new, f, indent=1)
        f.write("\n")
