"""Sequence packing on the CPU path: the packer's layout invariants, and the
claim that packing changes the layout, not the maths — a packed batch gives
the loss, the gradients and the optimizer trajectory of the padded batch
that holds the same sentence pairs."""

import random
from collections import Counter

import pytest
import torch

from transformer_amd.data import BatchedDataset, PackedBatch, pack_pairs
from transformer_amd.models import Transformer
from transformer_amd.ops import reference as R
from transformer_amd.runtime import Train

START, END = 98, 99


def _pairs(n, L, seed):
    """n encoded pairs, lengths uniform in 2..L (start/end included)."""
    rng = random.Random(seed)

    def sent():
        k = rng.randint(2, L)
        return [START] + [rng.randint(1, 90) for _ in range(k - 2)] + [END]
    return [(sent(), sent()) for _ in range(n)]


def _segments(pb, r):
    """[(id, src slice, tgt slice)] of row r, in order."""
    out = []
    k = 1
    while True:
        s = (pb.src_seg[r] == k).nonzero().flatten()
        t = (pb.tgt_seg[r] == k).nonzero().flatten()
        if len(s) == 0 and len(t) == 0:
            return out
        assert len(s) and len(t), "pair n must be segment n on both sides"
        out.append((k, s, t))
        k += 1


def _unpack(pb):
    """The (src, tgt) pairs a PackedBatch holds, checking every layout
    invariant on the way."""
    pairs = []
    assert isinstance(pb, PackedBatch)
    for name in ("src_seg", "src_pos", "tgt_seg", "tgt_pos"):
        assert getattr(pb, name).dtype == torch.int32, name
    for r in range(pb.src.shape[0]):
        segs = _segments(pb, r)
        assert segs, "no empty rows"
        for side_seg, side_pos, toks in ((pb.src_seg, pb.src_pos, pb.src),
                                         (pb.tgt_seg, pb.tgt_pos,
                                          pb.tar_inp)):
            ids = side_seg[r].tolist()
            n_real = sum(1 for i in ids if i)
            # ids 1..k, each contiguous and ascending, then zeros only
            assert ids[:n_real] == sorted(ids[:n_real]) and 0 not in ids[:n_real]
            assert set(ids[:n_real]) == set(range(1, len(segs) + 1))
            assert all(i == 0 for i in ids[n_real:])
            assert bool((toks[r, n_real:] == 0).all())
            assert bool((toks[r, :n_real] != 0).all())
            assert bool((side_pos[r, n_real:] == 0).all())
        assert bool(((pb.tar_real[r] != 0) == (pb.tgt_seg[r] != 0)).all())
        for k, s, t in segs:
            for idx, pos in ((s, pb.src_pos), (t, pb.tgt_pos)):
                assert idx.tolist() == list(range(int(idx[0]),
                                                  int(idx[0]) + len(idx)))
                assert pos[r, idx].tolist() == list(range(len(idx)))
            ti, tr = pb.tar_inp[r, t], pb.tar_real[r, t]
            # the shift happened inside the sentence
            assert torch.equal(ti[1:], tr[:-1])
            assert int(ti[0]) == START and int(tr[-1]) == END
            pairs.append((pb.src[r, s].tolist(),
                          ti.tolist() + [int(tr[-1])]))
    return pairs


def _key(pairs):
    return Counter((tuple(s), tuple(t)) for s, t in pairs)


@pytest.mark.parametrize("L", [16, 50])
@pytest.mark.parametrize("B", [1, 7, 64])
def test_packer_properties(B, L):
    pairs = _pairs(B, L, seed=B * 100 + L)
    pb = pack_pairs(pairs, L)
    for t in pb:
        assert t.shape == (pb.src.shape[0], L)      # width exactly L
    assert _key(_unpack(pb)) == _key(pairs)          # each pair exactly once
    assert pb.src.shape[0] <= B
    again = pack_pairs(pairs, L)
    assert all(torch.equal(a, b) for a, b in zip(pb, again))
    used = [(int((pb.src_seg[r] != 0).sum()), int((pb.tgt_seg[r] != 0).sum()))
            for r in range(pb.src.shape[0])]
    assert pb.real_tokens() == sum(a + b for a, b in used)


def test_packer_rejects_oversize_pair():
    with pytest.raises(ValueError):
        pack_pairs([([START] + [5] * 20 + [END], [START, END])], 16)


@pytest.mark.parametrize("L", [16, 50])
@pytest.mark.parametrize("world", [1, 2])
def test_packed_loader_draws_the_unpacked_loaders_pairs(world, L):
    pairs = _pairs(45, L, seed=L)       # 45 = 5 batches of 8 + a tail of 5
    for rank in range(world):
        kw = dict(batch_size=8, shuffle=True, seed=3, rank=rank,
                  world_size=world)
        plain = BatchedDataset(pairs, **kw)
        packed = BatchedDataset(pairs, pack_width=L, **kw)
        packed2 = BatchedDataset(pairs, pack_width=L, **kw)
        assert len(plain) == len(packed)
        for ep in range(2):
            for ds in (plain, packed, packed2):
                ds.set_epoch(ep)
            a, b, c = list(plain), list(packed), list(packed2)
            assert len(a) == len(b) == len(c)
            for (src, tar), pb, pb2 in zip(a, b, c):
                want = [(s[s != 0].tolist(), t[t != 0].tolist())
                        for s, t in zip(src, tar)]
                assert _key(_unpack(pb)) == _key(want)
                assert pb.src.shape[1] == L
                assert pb.src.shape[0] <= src.shape[0]
                assert all(torch.equal(x, y) for x, y in zip(pb, pb2))


# ---------------------------------------------------------------------------
# model equivalence, fp32 CPU path
# ---------------------------------------------------------------------------

def _tiny(seed=0):
    torch.manual_seed(seed)
    return Transformer(num_layers=2, d_model=32, num_heads=2, dff=64,
                       input_vocab_size=100, target_vocab_size=100, rate=0.0,
                       max_position=64)


def _nine_pairs():
    """9 pairs; source body lengths 1..12, target another order of them."""
    rng = random.Random(5)
    sl = [1, 2, 3, 5, 7, 8, 10, 11, 12]
    tl = [12, 1, 9, 4, 2, 11, 6, 3, 7]
    mk = lambda k: [START] + [rng.randint(1, 90) for _ in range(k)] + [END]
    return [(mk(a), mk(b)) for a, b in zip(sl, tl)]


def _padded(pairs):
    def pad(seqs):
        out = torch.zeros(len(seqs), max(map(len, seqs)), dtype=torch.int64)
        for i, s in enumerate(seqs):
            out[i, :len(s)] = torch.tensor(s)
        return out
    return pad([p[0] for p in pairs]), pad([p[1] for p in pairs])


def _loss_and_grads(model, batch, B):
    model.zero_grad()
    if isinstance(batch, PackedBatch):
        logits, _ = model(batch, training=True)
        real = batch.tar_real
    else:
        src, tar = batch
        logits, _ = model((src, tar[:, :-1].contiguous()), training=True)
        real = tar[:, 1:].contiguous()
    loss = R.masked_cross_entropy(logits, real, B)
    loss.backward()
    return loss.detach(), {n: p.grad.clone()
                           for n, p in model.named_parameters()}


@pytest.mark.parametrize("L", [16, 30])
def test_packed_loss_and_gradients_equal_padded(L):
    """Both sides are fp32 and hold the same terms in another summation
    order, so torch.testing.assert_close's fp32 defaults (rtol 1.3e-6, atol
    1e-5) are the bound."""
    pairs = _nine_pairs()
    model = _tiny()
    pb = pack_pairs(pairs, L)
    assert pb.src.shape[0] < len(pairs)          # really several per row
    l0, g0 = _loss_and_grads(model, _padded(pairs), len(pairs))
    l1, g1 = _loss_and_grads(model, pb, len(pairs))
    torch.testing.assert_close(l1, l0)
    assert set(g0) == set(g1)
    for n in g0:
        torch.testing.assert_close(g1[n], g0[n], msg=lambda m: f"{n}: {m}")


def test_eager_segment_semantics():
    """CPU attention with ids: id-0 query rows give exact zeros and take no
    gradient; a sentence's output does not depend on its row-mates."""
    from transformer_amd import ops
    torch.manual_seed(1)
    B, S, H, dh = 1, 12, 2, 8
    seg = torch.tensor([[1] * 5 + [2] * 4 + [0] * 3], dtype=torch.int32)
    q, k, v = (torch.randn(B, S, H, dh, requires_grad=True) for _ in range(3))
    o = ops.fused_attention(q, k, v, causal=True, q_seg=seg, kv_seg=seg)
    assert bool((o[:, 9:] == 0).all())
    o.sum().backward()
    assert bool((q.grad[:, 9:] == 0).all())
    assert bool((k.grad[:, 9:] == 0).all()) and bool((v.grad[:, 9:] == 0).all())
    alone = ops.fused_attention(q[:, 5:9], k[:, 5:9], v[:, 5:9], causal=True)
    torch.testing.assert_close(o[:, 5:9], alone)
    m = R.create_segment_mask(seg, seg, causal=True)
    assert m.shape == (B, 1, S, S)
    assert m[0, 0, 6, 5] == 0 and m[0, 0, 6, 7] == 1 and m[0, 0, 6, 4] == 1
    assert bool((m[0, 0, 9:] == 1).all())


# ---------------------------------------------------------------------------
# train-step parity
# ---------------------------------------------------------------------------

class Tok:
    vocab_size = 98

    def encode(self, s):
        return [5, 6, 7]

    def decode(self, ids):
        return "x"


def _run_steps(tmp_path, tag, batches, accum):
    tr = Train(1, False, _tiny(), Tok(), Tok(), 9, None, None, 2,
               str(tmp_path / tag), 32, warmup_steps=10,
               grad_accum_steps=accum)
    losses = [float(tr.train_step(b).detach()) for b in batches]
    return losses, tr


@pytest.mark.parametrize("accum", [1, 2])
def test_train_step_parity(tmp_path, accum):
    """Three optimizer steps, packed against unpacked, from the same initial
    weights: same losses (fp32 assert_close defaults), same step count, same
    token-weighted accuracy."""
    all_pairs = _pairs(27, 14, seed=2)
    steps = [all_pairs[i * 9:(i + 1) * 9] for i in range(3)]
    plain = [_padded(p) for p in steps]
    packed = [pack_pairs(p, 16) for p in steps]
    l0, t0 = _run_steps(tmp_path, "plain", plain, 1)
    l1, t1 = _run_steps(tmp_path, f"packed{accum}", packed, accum)
    assert t0.optimizer.step_count == t1.optimizer.step_count == 3
    print("losses", l0, l1)
    torch.testing.assert_close(torch.tensor(l1), torch.tensor(l0))
    assert t0.train_accuracy.result() == pytest.approx(
        t1.train_accuracy.result(), abs=1e-6)


# ---------------------------------------------------------------------------
# flags
# ---------------------------------------------------------------------------

def test_flag_default_off_and_synthetic_is_an_error(capsys):
    from transformer_amd.config import parse_flags, flags_dict
    assert parse_flags([]).pack_sequences is False
    assert flags_dict(parse_flags([]))["pack_sequences"] is False
    assert parse_flags(["--pack_sequences"]).pack_sequences is True
    with pytest.raises(SystemExit):
        parse_flags(["--pack_sequences", "--synthetic_data"])
    import train
    with pytest.raises(ValueError, match="pack_sequences"):
        train.main(**dict(flags_dict(parse_flags([])), pack_sequences=True,
                          synthetic_data=True))


def test_packed_capture_is_refused_at_startup(tmp_path, monkeypatch):
    """The captured (enable_function) step has no packed buffers: a run that
    would capture must fail when the trainer is built, not mid-epoch."""
    monkeypatch.setattr(Train, "_graph_eligible", lambda self: True)
    with pytest.raises(ValueError, match="enable_function"):
        Train(1, True, _tiny(), Tok(), Tok(), 9, None, None, 2,
              str(tmp_path / "ck"), 32, pack_sequences=True)
    monkeypatch.setattr(Train, "_graph_eligible", lambda self: False)
    Train(1, True, _tiny(), Tok(), Tok(), 9, None, None, 2,
          str(tmp_path / "ck2"), 32, pack_sequences=True)
