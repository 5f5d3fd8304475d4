"""Beam search without a GPU: reference ops, decoder, serve.py options."""

import pytest
import torch


def test_reference_beam_topk_matches_brute_force():
    """V = 7, K = 3, B = 2; sentence 0 has a finished beam, sentence 1 a
    dead one."""
    from transformer_amd.ops import reference as R
    B, K, V, end_id = 2, 3, 7, 4
    torch.manual_seed(0)
    logits = torch.randn(B * K, V) * 2
    scores = -torch.rand(B, K)
    finished = torch.zeros(B, K, dtype=torch.uint8)
    finished[0, 1] = 1
    scores[1, 2] = float("-inf")
    lens = torch.randint(1, 5, (B, K), dtype=torch.int32)
    tok, parent, src_row, sc, fin, ln = R.beam_topk(logits, scores, finished,
                                                    lens, end_id)
    lp = torch.log_softmax(logits, dim=-1).view(B, K, V)
    for b in range(B):
        cands = []                      # (-score, flat index, k, v)
        for k in range(K):
            if finished[b, k]:
                cands.append((-float(scores[b, k]), k * V, k, 0))
            elif scores[b, k] > float("-inf"):
                cands += [(-float(scores[b, k] + lp[b, k, v]), k * V + v, k, v)
                          for v in range(V)]
        for j, (neg, _, k, v) in enumerate(sorted(cands)[:K]):
            o = b * K + j
            f = bool(finished[b, k])
            assert (int(tok[o]), int(parent[b, j]), int(src_row[o])) == \
                (v, k, b * K + k)
            assert float(sc[b, j]) == -neg
            assert bool(fin[b, j]) == (f or v == end_id)
            assert int(ln[b, j]) == int(lens[b, k]) + (0 if f else 1)


def test_cpu_beam_size_1_is_greedy():
    from transformer_amd.models import Transformer
    from transformer_amd.models.transformer import (beam_search_decode,
                                                    greedy_decode)
    torch.manual_seed(1)
    model = Transformer(num_layers=1, d_model=16, num_heads=2, dff=32,
                        input_vocab_size=30, target_vocab_size=30, rate=0.0,
                        max_position=32).eval()
    inp = torch.randint(2, 28, (3, 6))
    inp[2, 4:] = 0
    ref = greedy_decode(model, inp, 28, 29, max_len=8)
    hyps, scores = beam_search_decode(model, inp, 28, 29, beam_size=1,
                                      max_len=8)
    assert hyps.shape[:2] == (3, 1) and scores.shape == (3, 1)
    n = min(ref.shape[1], hyps.shape[2])
    assert torch.equal(hyps[:, 0, :n], ref[:, :n])
    wide, ws = beam_search_decode(model, inp, 28, 29, beam_size=3, max_len=8)
    assert bool((ws[:, :-1] >= ws[:, 1:]).all())
    assert all(len({tuple(h) for h in s}) == 3 for s in wide.tolist())


def test_serve_beam_arguments():
    import serve
    assert serve.parse_args([]).beam_size == 1
    args = serve.parse_args(["--beam_size", "4", "--length_penalty", "0.6"])
    assert (args.beam_size, args.length_penalty) == (4, 0.6)
    assert [serve.clamp_beam_size(n) for n in (-3, 1, 5, 99)] == [1, 1, 5, 8]


def test_serve_beam_endpoint(tmp_path, toy_corpus):
    pytest.importorskip("fastapi")
    from fastapi.testclient import TestClient

    from transformer_amd.data.dataset import load_dataset
    from transformer_amd.models import Transformer
    from transformer_amd.runtime import export_model
    import serve

    _, _, src_tok, tgt_tok = load_dataset(
        toy_corpus, str(tmp_path / "sv"), str(tmp_path / "tv"),
        sequence_length=50, batch_size=4, seed=1)
    torch.manual_seed(0)
    cfg = dict(num_layers=1, d_model=16, num_heads=2, dff=32,
               input_vocab_size=src_tok.vocab_size + 2,
               target_vocab_size=tgt_tok.vocab_size + 2)
    model = Transformer(rate=0.0, max_position=64, **cfg)
    export_model(model, str(tmp_path / "model"),
                 dict(cfg, dropout_rate=0.0, max_position=64))
    client = TestClient(serve.build_app(
        str(tmp_path / "model"), str(tmp_path / "sv"), str(tmp_path / "tv")))
    greedy = client.post("/translate",
                         json={"text": "one two", "max_len": 4}).json()
    assert greedy["score"] is None
    beam = client.post("/translate", json={"text": "one two", "max_len": 4,
                                           "beam_size": 99}).json()
    assert isinstance(beam["tokens"], list) and "text" in beam
    assert isinstance(beam["score"], float) and beam["score"] <= 0.0
