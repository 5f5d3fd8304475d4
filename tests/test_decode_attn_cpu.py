"""CPU wiring of the decode-attention ops: the reference implementation
against plain attention on the prefix, and greedy_decode(fused_attn=True)."""

import pytest
import torch

from transformer_amd import ops
from transformer_amd.ops import reference as R


@pytest.mark.parametrize("lens", [[0, 3, 6], [7, 7, 8]])
def test_reference_self_matches_prefix_attention(lens):
    torch.manual_seed(0)
    B, H, dh, Lmax = 3, 2, 8, 8
    qkv = torch.randn(B, 1, 3, H, dh)
    cache = torch.randn(B, Lmax, 2, H, dh)
    before = cache.clone()
    kv_len = torch.tensor(lens, dtype=torch.int32)
    ws = ops.decode_attention_workspace(B, H, dh, Lmax, "cpu")
    out = ops.decode_attention_self(qkv, cache, kv_len, ws)
    assert kv_len.tolist() == lens
    for b, n in enumerate(lens):
        full = n >= Lmax
        want = before[b].clone()
        if not full:
            want[n] = qkv[b, 0, 1:3]
        assert torch.equal(cache[b], want)
        kv = torch.cat([before[b, :n], qkv[b, :, 1:3]])       # (n+1,2,H,dh)
        ref = R.scaled_dot_product_attention(
            qkv[b, :, 0].permute(1, 0, 2), kv[:, 0].permute(1, 0, 2),
            kv[:, 1].permute(1, 0, 2)).permute(1, 0, 2)
        torch.testing.assert_close(out[b], ref, rtol=1e-6, atol=1e-6)


def test_reference_cross_matches_fused_attention():
    torch.manual_seed(1)
    B, H, dh, Sk = 2, 2, 8, 5
    q = torch.randn(B, 1, H, dh)
    kv = torch.randn(B, Sk, 2, H, dh)
    pad = torch.zeros(B, Sk, dtype=torch.uint8)
    pad[1, 3:] = 1
    out = ops.decode_attention_cross(q, kv, pad, None)
    ref = ops.fused_attention(q, kv[:, :, 0], kv[:, :, 1], kv_pad=pad)
    torch.testing.assert_close(out, ref, rtol=1e-6, atol=1e-6)


def test_greedy_decode_fused_attn_cpu():
    from transformer_amd.models import Transformer
    from transformer_amd.models.transformer import greedy_decode

    torch.manual_seed(3)
    model = Transformer(num_layers=2, d_model=32, num_heads=4, dff=64,
                        input_vocab_size=52, target_vocab_size=52, rate=0.0,
                        max_position=32)
    model.eval()
    inp = torch.randint(2, 50, (2, 9))
    inp[1, 6:] = 0
    plain = greedy_decode(model, inp, 50, 51, max_len=8)
    fused = greedy_decode(model, inp, 50, 51, max_len=8, fused_attn=True)
    assert torch.equal(plain, fused)
