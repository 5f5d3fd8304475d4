"""CPU wiring of the LayerNorm-in-the-consumer decode linear: the op against
its residual_layernorm + linear_rows composition, and
greedy_decode(skinny_preln=True)."""

import pytest
import torch

from transformer_amd import ops


@pytest.mark.parametrize("bias,act", [(True, "relu"), (False, None)])
def test_op_matches_composition(bias, act):
    torch.manual_seed(0)
    pre, res = torch.randn(2, 3, 16), torch.randn(2, 3, 16)
    gamma, beta = torch.randn(16), torch.randn(16)
    w, b = torch.randn(24, 16), torch.randn(24) if bias else None
    xn, y = ops.residual_layernorm_linear(pre, res, gamma, beta, 1e-6, w, b,
                                          act)
    ref = ops.residual_layernorm(pre, res, gamma, beta, 1e-6)
    assert torch.equal(xn, ref)
    assert torch.equal(y, ops.linear_rows(ref, w, b, act))


def _model():
    from transformer_amd.models import Transformer
    torch.manual_seed(3)
    model = Transformer(num_layers=2, d_model=32, num_heads=4, dff=64,
                        input_vocab_size=52, target_vocab_size=52, rate=0.0,
                        max_position=32)
    model.eval()
    inp = torch.randint(2, 50, (2, 9))
    inp[1, 6:] = 0
    return model, inp


def test_greedy_decode_skinny_preln_cpu():
    from transformer_amd.models.transformer import greedy_decode
    model, inp = _model()
    plain = greedy_decode(model, inp, 50, 51, max_len=8)
    assert torch.equal(plain, greedy_decode(model, inp, 50, 51, max_len=8,
                                            skinny_linear=True,
                                            skinny_preln=True))


def test_skinny_preln_excludes_skinny_ln():
    from transformer_amd.models.transformer import greedy_decode
    model, inp = _model()
    with pytest.raises(ValueError):
        greedy_decode(model, inp, 50, 51, max_len=8, skinny_linear=True,
                      skinny_ln=True, skinny_preln=True)
