"""Segment-masked attention kernels and the packed model on the GPU.

Oracle: ops/reference.py scaled_dot_product_attention in fp32 with the dense
create_segment_mask.  The oracle's additive rule gives id-0 query rows
uniform attention where the kernels define zeros, so O is compared at rows
with id != 0 and the gradients with dO zeroed at id-0 rows; the id-0 rows
have tests of their own."""

import math

import pytest
import torch

from _gpu_bounds import _check_pair

pytestmark = pytest.mark.gpu

FWD_TOL, BWD_TOL = 0.04, 0.06      # the attention tests' own tolerances


def _ext():
    from transformer_amd.ops import ext
    return ext()


def assert_close(got, ref, tol, name=""):
    got = got.float().cpu()
    ref = ref.float().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    scale = ref.abs().max().clamp(min=1.0)
    err = (got - ref).abs().max() / scale
    print(f"{name}: rel-max err {err:.4f}")
    assert err < tol, f"{name}: rel-max err {err:.4f} (tol {tol})"


def _ids(rows, S):
    """rows: per batch row a list of segment lengths -> (B,S) int32 ids."""
    out = torch.zeros(len(rows), S, dtype=torch.int32)
    for b, lens in enumerate(rows):
        o = 0
        for k, n in enumerate(lens, start=1):
            out[b, o:o + n] = k
            o += n
        assert o <= S
    return out.cuda()


def _oracle(q, k, v, q_seg, kv_seg, causal):
    import transformer_amd.ops.reference as R
    qt, kt, vt = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    mask = R.create_segment_mask(q_seg, kv_seg, causal)
    return R.scaled_dot_product_attention(qt, kt, vt, mask).permute(0, 2, 1, 3)


def _rand(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g).bfloat16()


def _check_case(q, k, v, do, q_seg, kv_seg, causal, run, name):
    """run(q, k, v, do) -> (o, lse, dq, dk, dv) from the kernels."""
    live = (q_seg != 0)[:, :, None, None]
    do = do * live                                  # dO = 0 at id-0 rows
    o, lse, dq, dk, dv = run(q, k, v, do)
    qf, kf, vf = (t.float().requires_grad_(True) for t in (q, k, v))
    ref = _oracle(qf, kf, vf, q_seg, kv_seg, causal)
    ref.backward(do.float())
    assert_close(o * live, ref.detach() * live, FWD_TOL, f"{name} O")
    assert_close(dq, qf.grad, BWD_TOL, f"{name} dQ")
    assert_close(dk, kf.grad, BWD_TOL, f"{name} dK")
    assert_close(dv, vf.grad, BWD_TOL, f"{name} dV")
    # id-0 rows: exact zeros, everything finite
    dead = ~live.expand_as(o)
    assert bool((o[dead] == 0).all()), f"{name}: O at id-0 rows"
    assert bool((dq[dead] == 0).all()), f"{name}: dQ at id-0 rows"
    kdead = (kv_seg == 0)[:, :, None, None].expand_as(dk)
    assert bool((dk[kdead] == 0).all()) and bool((dv[kdead] == 0).all())
    for t in (o, lse, dq, dk, dv):
        assert bool(torch.isfinite(t.float()).all()), name


def _run_plain(q_seg, kv_seg, causal):
    def run(q, k, v, do):
        E = _ext()
        scale = 1.0 / math.sqrt(q.shape[-1])
        o, lse = E.attn_fwd_seg(q, k, v, q_seg, kv_seg, causal, scale)
        dq, dk, dv = E.attn_bwd_seg(q, k, v, o, do.contiguous(), lse, q_seg,
                                    kv_seg, causal, scale, 0)
        return o, lse, dq, dk, dv
    return run


# self-attention layout: a length-1 segment, a segment holding a whole 64-key
# tile, boundaries off every multiple of 16; one full row; one all-pad row
SELF_ROWS, SELF_S = [[3, 1, 150, 30], [200], []], 200
# cross layout: target lengths / source lengths, Sq != Sk
CROSS_T, CROSS_S, SQ, SK = [[5, 40, 20], [70], []], [[60, 7, 70], [150], []], 70, 150


@pytest.mark.parametrize("dh", [64, 128])
@pytest.mark.parametrize("causal", [False, True])
def test_self_attention_vs_oracle(dh, causal):
    g = torch.Generator(device="cuda").manual_seed(dh + causal)
    B, S, H = 3, SELF_S, 2
    seg = _ids(SELF_ROWS, S)
    q, k, v, do = (_rand(g, B, S, H, dh) for _ in range(4))
    _check_case(q, k, v, do, seg, seg, causal, _run_plain(seg, seg, causal),
                f"self dh{dh} causal{causal}")


@pytest.mark.parametrize("dh", [64, 128])
def test_cross_attention_vs_oracle(dh):
    g = torch.Generator(device="cuda").manual_seed(dh)
    B, H = 3, 2
    qs, ks = _ids(CROSS_T, SQ), _ids(CROSS_S, SK)
    q, do = _rand(g, B, SQ, H, dh), _rand(g, B, SQ, H, dh)
    k, v = _rand(g, B, SK, H, dh), _rand(g, B, SK, H, dh)
    _check_case(q, k, v, do, qs, ks, False, _run_plain(qs, ks, False),
                f"cross dh{dh}")


def test_packed_qkv_mode_through_autograd():
    """Mode 1: strided q/k/v slots of one (B,S,3,H,dh) tensor, one dQKV."""
    from transformer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(7)
    B, S, H, dh = 3, SELF_S, 2, 64
    seg = _ids(SELF_ROWS, S)
    qkv = _rand(g, B, S, 3, H, dh)
    do = _rand(g, B, S, H, dh)

    def run(q, k, v, do):
        x = qkv.clone().requires_grad_(True)
        o = ops.self_attention(x, causal=True, q_seg=seg, kv_seg=seg)
        o.backward(do)
        dq, dk, dv = x.grad.unbind(dim=2)
        return o.detach(), torch.zeros(1), dq, dk, dv
    q, k, v = qkv.unbind(dim=2)
    _check_case(q, k, v, do, seg, seg, True, run, "packed-QKV")


def test_packed_kv_mode_through_autograd():
    """Mode 2: q + strided k/v slots of one (B,Sk,2,H,dh) tensor."""
    from transformer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(8)
    B, H, dh = 3, 2, 64
    qs, ks = _ids(CROSS_T, SQ), _ids(CROSS_S, SK)
    q0, do = _rand(g, B, SQ, H, dh), _rand(g, B, SQ, H, dh)
    kv = _rand(g, B, SK, 2, H, dh)

    def run(q, k, v, do):
        qq = q0.clone().requires_grad_(True)
        x = kv.clone().requires_grad_(True)
        o = ops.cross_attention(qq, x, q_seg=qs, kv_seg=ks)
        o.backward(do)
        dk, dv = x.grad.unbind(dim=2)
        return o.detach(), torch.zeros(1), qq.grad, dk, dv
    k, v = kv.unbind(dim=2)
    _check_case(q0, k, v, do, qs, ks, False, run, "packed-KV")


def test_long_row_runs_the_qt64_backward():
    """Sq, Sk >= 1024 dispatches the 64-row backward tiles."""
    g = torch.Generator(device="cuda").manual_seed(9)
    B, S, H, dh = 1, 1100, 1, 64
    seg = _ids([[300, 7, 500, 64, 129, 70]], S)     # 30 pad
    q, k, v, do = (_rand(g, B, S, H, dh) for _ in range(4))
    _check_case(q, k, v, do, seg, seg, True, _run_plain(seg, seg, True),
                "S1100 causal")


@pytest.mark.parametrize("causal", [False, True])
def test_isolation_is_bitwise(causal):
    """NaN in every Q/K/V/dO element of segment [64,192) — aligned to every
    32- and 64-row tile — must leave all other rows finite and bit-identical:
    0 * NaN is NaN, so this holds only if those tiles are never multiplied,
    i.e. skipped, not merely masked."""
    g = torch.Generator(device="cuda").manual_seed(10)
    B, S, H, dh = 1, 256, 2, 64
    seg = _ids([[40, 24, 128, 58]], S)              # 6 pad
    q, k, v, do = (_rand(g, B, S, H, dh) for _ in range(4))
    run = _run_plain(seg, seg, causal)
    clean = run(q, k, v, do)
    for t in (q, k, v, do):
        t[:, 64:192] = float("nan")
    dirty = run(q, k, v, do)
    keep = torch.ones(S, dtype=torch.bool, device="cuda")
    keep[64:192] = False
    for name, a, b in zip(("O", "LSE", "dQ", "dK", "dV"), clean, dirty):
        a, b = (a[:, :, keep] if name == "LSE" else a[:, keep]), \
               (b[:, :, keep] if name == "LSE" else b[:, keep])
        assert bool(torch.isfinite(b.float()).all()), f"{name} not finite"
        assert torch.equal(a, b), f"{name} changed outside the NaN segment"


def test_embedding_positions():
    """positions against the oracle, bit-exact: d = 64 makes sqrt(d) a power
    of two, so w * sqrt(d) is exact in fp32 and the kernel's
    multiply-add equals the oracle's separate multiply and add whether or
    not the compiler fuses it.  positions = column index reproduces the
    kernel without positions bit for bit."""
    import transformer_amd.ops.reference as R
    from transformer_amd import ops
    g = torch.Generator(device="cuda").manual_seed(11)
    V, d, B, S, P = 50, 64, 3, 21, 40
    tokens = torch.randint(0, V, (B, S), device="cuda", generator=g)
    w, pe = _rand(g, V, d), _rand(g, P, d)
    pos = torch.zeros(B, S, dtype=torch.int32, device="cuda")
    pos[0] = torch.arange(S)
    pos[1] = torch.cat([torch.arange(4), torch.arange(10), torch.arange(7)])
    pos[2, :5] = torch.arange(5)
    pos[2, 5] = P - 1
    y = ops.embedding_scale_pe(tokens, w, pe, positions=pos)
    ref = R.embedding_scale_pe(tokens, w.float(), pe[None].float(), pos)
    assert torch.equal(y, ref.bfloat16())
    cols = torch.arange(S, dtype=torch.int32, device="cuda").expand(B, S)
    assert torch.equal(ops.embedding_scale_pe(tokens, w, pe, positions=cols),
                       ops.embedding_scale_pe(tokens, w, pe))
    assert torch.equal(_ext().embed_pe_fwd(tokens, w, pe),
                       ops.embedding_scale_pe(tokens, w, pe))


def test_packed_model_matches_padded_model():
    """bf16 model, d=64: loss and flat gradient of a packed batch against the
    padded batch of the same 9 pairs.  Loss: two bf16-path roundings of one
    sum (_check_pair).  Gradients: the kernel tests' rel-max assert_close.
    test_gpu_flat_parity.py itself has no rel-max figure (it demands
    bit-equality or _check_pair between runs of the SAME kernels on the SAME
    operands); here the two runs feed differently shaped GEMMs and attention
    tiles, so intermediate bf16 roundings differ and the bound is the
    loosest kernel tolerance on the path, the attention backward's 0.06."""
    import random
    from transformer_amd.data import pack_pairs
    from transformer_amd.models import Transformer
    from transformer_amd import ops
    rng = random.Random(5)
    mk = lambda n: [98] + [rng.randint(1, 90) for _ in range(n)] + [99]
    pairs = [(mk(a), mk(b)) for a, b in zip([1, 2, 3, 5, 7, 8, 10, 11, 12],
                                            [12, 1, 9, 4, 2, 11, 6, 3, 7])]
    torch.manual_seed(0)
    model = Transformer(num_layers=2, d_model=64, num_heads=2, dff=128,
                        input_vocab_size=100, target_vocab_size=100, rate=0.0,
                        max_position=64).to("cuda", torch.bfloat16)

    def pad(seqs):
        out = torch.zeros(len(seqs), max(map(len, seqs)), dtype=torch.int64)
        for i, s in enumerate(seqs):
            out[i, :len(s)] = torch.tensor(s)
        return out.cuda()

    def grads():
        return torch.cat([p.grad.float().flatten()
                          for p in model.parameters()])
    src, tar = pad([p[0] for p in pairs]), pad([p[1] for p in pairs])
    logits, _ = model((src, tar[:, :-1].contiguous()), training=True)
    l0 = ops.masked_cross_entropy(logits, tar[:, 1:].contiguous(), 9)
    l0.backward()
    g0 = grads()
    model.zero_grad()
    pb = pack_pairs(pairs, 32).to("cuda")
    assert pb.src.shape[0] < 9
    logits, _ = model(pb, training=True)
    l1 = ops.masked_cross_entropy(logits, pb.tar_real, 9)
    l1.backward()
    g1 = grads()
    _check_pair(l1.detach().reshape(1), l0.detach().reshape(1), "loss")
    assert_close(g1, g0, BWD_TOL, "flat gradient")


def test_packed_train_step_and_capture_refusal(tmp_path):
    """Eager packed train_step runs on the GPU (flat path, HIP kernels);
    with the captured step selected the trainer refuses at construction."""
    from transformer_amd.data import pack_pairs
    from transformer_amd.models import Transformer
    from transformer_amd.runtime import Train

    class Tok:
        vocab_size = 98

        def encode(self, s):
            return [5, 6, 7]

    def model():
        torch.manual_seed(0)
        return Transformer(num_layers=1, d_model=64, num_heads=2, dff=128,
                           input_vocab_size=100, target_vocab_size=100,
                           rate=0.1, max_position=64).to("cuda",
                                                         torch.bfloat16)
    pairs = [([98, 5, 6, 99], [98, 7, 99]), ([98, 9, 99], [98, 4, 5, 6, 99]),
             ([98, 3, 99], [98, 8, 99])]
    pb = pack_pairs(pairs, 16)
    tr = Train(1, False, model(), Tok(), Tok(), 3, None, None, 2,
               str(tmp_path / "a"), 64, warmup_steps=10, use_flat=True,
               pack_sequences=True)
    losses = [float(tr.train_step(pb).detach()) for _ in range(3)]
    assert all(math.isfinite(x) for x in losses), losses
    assert tr.optimizer.step_count == 3
    with pytest.raises(ValueError, match="enable_function"):
        Train(1, True, model(), Tok(), Tok(), 3, None, None, 2,
              str(tmp_path / "b"), 64, use_flat=True, pack_sequences=True)
