"""LLaMA.prefill_batch at head size 64 (the two-layer MiniCPM-2B model of the other head-size-64 tests): fresh and continued prompts on
the matrix-core prompt kernel against the same calls on the mask form of the decode kernel (ZL_PREFILL_D64=0)."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def test_prefill_batch_d64_kernel_route_against_mask_route(dev, monkeypatch):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig.minicpm_2b()
    cfg.num_layers = 2
    model = LLaMA(cfg, QuantConfig(0, 0), dev).init_random(seed=3)
    model.token_embedding.mul_(0.1)
    g = torch.Generator().manual_seed(64)
    first = [torch.randint(0, cfg.vocab_size, (s,), generator=g, dtype=torch.int32) for s in (9, 70, 130)]
    more = [torch.randint(0, cfg.vocab_size, (s,), generator=g, dtype=torch.int32) for s in (5, 66)]

    def run():
        ctx = model.new_context(3, 256, 0)
        calls = []
        for logits in (model.prefill_batch(ctx, [0, 1, 2], first), model.prefill_batch(ctx, [0, 1], more, pos0=[9, 70])):
            calls.append((logits.float(), ctx.tokens.tolist(), ctx.positions.tolist(), ctx.valid_lens.tolist()))
        return calls

    new = run()
    assert not [k for k in model._bufs if isinstance(k, tuple) and k[0] == "prefill"]      # no mask was built on the kernel route
    monkeypatch.setenv("ZL_PREFILL_D64", "0")
    old = run()
    assert [k for k in model._bufs if isinstance(k, tuple) and k[0] == "prefill"]
    for call, ((ln, *state_n), (lo, *state_o)) in enumerate(zip(new, old)):
        assert torch.isfinite(ln).all() and torch.isfinite(lo).all()
        err = (ln - lo).abs().max().item() / lo.abs().max().item()
        print(f"head size 64, kernel route against mask route, call {call}: max |dlogit| / max |logit| = {err:.3e}")
        assert err <= 2e-2, (call, err)
        assert state_n == state_o, call
