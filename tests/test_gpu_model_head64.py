"""A GQA model with head size 64 (8 query heads on 2 kv heads, bf16, two layers): its decode steps run the matrix-core decode
attention of decode_attn_d64.hip inside zl_decode_attn_fused, and must agree with the prompt pass over the same tokens."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("prompt_lens", [(9,), (9, 70, 33)])
def test_gqa_head64_decode_steps_consistent_with_prefill(dev, prompt_lens):
    from zhilight_amd.llama import LLaMA, ModelConfig, QuantConfig
    cfg = ModelConfig(num_layers=2, dim_model=512, num_heads=8, dim_head=64, dim_ff=1024, vocab_size=1000, num_kv_heads=2,
                      rope_theta=10000.0, dtype="bfloat16")
    model = LLaMA(cfg, QuantConfig(0, 0), dev).init_random(seed=5)
    b = len(prompt_lens)
    g = torch.Generator().manual_seed(b)
    prompts = [torch.randint(0, cfg.vocab_size, (n,), dtype=torch.int32, generator=g).to(dev) for n in prompt_lens]
    whole, short = model.new_context(b, 128, 0), model.new_context(b, 128, 0)
    lp = torch.cat([model.prefill(whole, i, p).float().reshape(1, -1) for i, p in enumerate(prompts)])
    for i, p in enumerate(prompts):
        model.prefill(short, i, p[:-1])
    short.tokens.copy_(torch.stack([p[-1] for p in prompts]))            # the decode step re-feeds each prompt's last token
    bar = 3e-2                      # test_minicpm_shaped_model_prefill_consistent_with_decode's, of the decode logits' max
    for step in range(3):
        ld = model.encode(short).float().reshape(b, -1)
        assert torch.isfinite(lp).all() and torch.isfinite(ld).all()
        assert (lp - ld).abs().max().item() <= bar * ld.abs().max().item(), step
        nxt = lp.argmax(dim=-1).to(torch.int32)
        model.advance(short, nxt)
        if step:
            model.advance(whole, nxt)
        else:
            whole.tokens.copy_(nxt)                   # a prefilled context is already at its first decode step
        lp = model.encode(whole).float().reshape(b, -1)
