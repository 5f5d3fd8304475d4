"""Encoder-decoder Transformer, MI355X-first.

Capability parity with the reference model (reference Transformer.py:5-32,
Encoder.py, Decoder.py, Attention.py, point_ffn.py — SURVEY.md §2.1 C1-C10):
post-LN residuals, three attention variants (encoder self bidirectional+pad,
decoder causal+pad, cross q-len≠kv-len+pad), sinusoidal PE in the reference's
CONCAT layout, embedding ×√d, final linear logits head.

MI355X-first differences from the reference's structure (not behaviour):
  * QKV projections are packed into one fused MFMA GEMM;
    cross-attention packs KV.
  * Attention runs as one fused flash-style HIP kernel in (B,S,H,dh) layout —
    no head split/merge transposes, no S×S materialization.
  * Residual-add + LayerNorm are fused (K9); embedding+scale+PE fused (K10).
  * Attention weights are only materialized in inspection mode
    (`return_attention=True`, eager path) — SURVEY.md §8 Q13.

On CPU the same modules run the fp32 reference math (ops/reference.py), which
is the numerics oracle for every kernel.
"""

from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import ops
from ..ops import reference as R


def _glorot(out_f: int, in_f: int) -> torch.Tensor:
    """Keras Dense default initializer (glorot_uniform), matching the
    reference's tf.keras.layers.Dense (reference Attention.py:46-50)."""
    limit = math.sqrt(6.0 / (in_f + out_f))
    return torch.empty(out_f, in_f).uniform_(-limit, limit)


class SelfAttention(nn.Module):
    """Multi-head self-attention with packed QKV projection (C2 / K1)."""

    def __init__(self, d_model: int, num_heads: int):
        super().__init__()
        assert d_model % num_heads == 0
        self.d_model, self.num_heads = d_model, num_heads
        self.depth = d_model // num_heads
        w = torch.cat([_glorot(d_model, d_model) for _ in range(3)], dim=0)
        self.w_qkv = nn.Parameter(w)              # (3d, d)
        self.b_qkv = nn.Parameter(torch.zeros(3 * d_model))
        self.w_o = nn.Parameter(_glorot(d_model, d_model))
        self.b_o = nn.Parameter(torch.zeros(d_model))

    def forward(self, x, kv_pad=None, causal=False, return_weights=False,
                project=True, seg=None):
        """project=False returns the merged heads BEFORE the output
        projection — the layer then runs w_o/b_o fused with its
        dropout + residual LayerNorm (one autograd node).  seg: (B,S)
        segment ids of a packed row (replaces kv_pad)."""
        B, S, d = x.shape
        qkv = ops.linear(x, self.w_qkv, self.b_qkv)          # (B,S,3d)
        qkv = qkv.view(B, S, 3, self.num_heads, self.depth)
        # packed path: the attention kernels read q/k/v slots through strides
        # and backward emits one packed dQKV (no copies)
        if seg is not None:
            out = ops.self_attention(qkv, causal=causal,
                                     return_weights=return_weights,
                                     q_seg=seg, kv_seg=seg)
        else:
            out = ops.self_attention(qkv, kv_pad=kv_pad, causal=causal,
                                     return_weights=return_weights)
        if return_weights:
            out, w = out
        out = out.reshape(B, S, d)
        if project:
            out = ops.linear(out, self.w_o, self.b_o)
        return (out, w) if return_weights else (out, None)


class CrossAttention(nn.Module):
    """Decoder-encoder cross attention with packed KV projection (C2)."""

    def __init__(self, d_model: int, num_heads: int):
        super().__init__()
        assert d_model % num_heads == 0
        self.d_model, self.num_heads = d_model, num_heads
        self.depth = d_model // num_heads
        self.w_q = nn.Parameter(_glorot(d_model, d_model))
        self.b_q = nn.Parameter(torch.zeros(d_model))
        w = torch.cat([_glorot(d_model, d_model) for _ in range(2)], dim=0)
        self.w_kv = nn.Parameter(w)               # (2d, d)
        self.b_kv = nn.Parameter(torch.zeros(2 * d_model))
        self.w_o = nn.Parameter(_glorot(d_model, d_model))
        self.b_o = nn.Parameter(torch.zeros(d_model))

    def forward(self, x, enc_output, kv_pad=None, return_weights=False,
                project=True, q_seg=None, kv_seg=None):
        B, Sq, d = x.shape
        Sk = enc_output.shape[1]
        q = ops.linear(x, self.w_q, self.b_q).view(B, Sq, self.num_heads, self.depth)
        kv = ops.linear(enc_output, self.w_kv, self.b_kv)
        kv = kv.view(B, Sk, 2, self.num_heads, self.depth)
        if q_seg is not None:
            out = ops.cross_attention(q, kv, return_weights=return_weights,
                                      q_seg=q_seg, kv_seg=kv_seg)
        else:
            out = ops.cross_attention(q, kv, kv_pad=kv_pad,
                                      return_weights=return_weights)
        if return_weights:
            out, w = out
        out = out.reshape(B, Sq, d)
        if project:
            out = ops.linear(out, self.w_o, self.b_o)
        return (out, w) if return_weights else (out, None)


class FeedForward(nn.Module):
    """Position-wise FFN: Dense(dff, relu) -> Dense(d) (C3 / K8), ReLU fused
    into the first GEMM's epilogue."""

    def __init__(self, d_model: int, dff: int):
        super().__init__()
        self.w1 = nn.Parameter(_glorot(dff, d_model))
        self.b1 = nn.Parameter(torch.zeros(dff))
        self.w2 = nn.Parameter(_glorot(d_model, dff))
        self.b2 = nn.Parameter(torch.zeros(d_model))

    def forward(self, x):
        h = ops.linear(x, self.w1, self.b1, activation="relu")
        return ops.linear(h, self.w2, self.b2)


def _proj_ln(mha, heads, res, ln, rate, training):
    """LN(dropout(heads @ w_o^T + b_o) + res)."""
    return ops.linear_dropout_residual_layernorm(
        heads, mha.w_o, mha.b_o, res, ln.gamma, ln.beta, rate, training,
        ln.eps)


def _ffn_ln(ffn, x, ln, rate, training):
    """LN(dropout(ffn(x)) + x)."""
    return ops.ffn_dropout_residual_layernorm(
        x, ffn.w1, ffn.b1, ffn.w2, ffn.b2, ln.gamma, ln.beta, rate, training,
        ln.eps)


class _LN(nn.Module):
    def __init__(self, d_model: int, eps: float = 1e-6):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(d_model))
        self.beta = nn.Parameter(torch.zeros(d_model))
        self.eps = eps


class EncoderLayer(nn.Module):
    """MHA -> dropout -> LN(x+.) -> FFN -> dropout -> LN(.+.) (C6,
    reference Encoder.py:6-29, post-LN)."""

    def __init__(self, d_model, num_heads, dff, rate=0.1):
        super().__init__()
        self.mha = SelfAttention(d_model, num_heads)
        self.ffn = FeedForward(d_model, dff)
        self.ln1 = _LN(d_model)
        self.ln2 = _LN(d_model)
        self.rate = rate

    def forward(self, x, kv_pad, training, seg=None):
        heads, _ = self.mha(x, kv_pad=kv_pad, causal=False, project=False,
                            seg=seg)
        out1 = _proj_ln(self.mha, heads, x, self.ln1, self.rate, training)
        return _ffn_ln(self.ffn, out1, self.ln2, self.rate, training)


class DecoderLayer(nn.Module):
    """masked self-MHA -> cross-MHA -> FFN, each with dropout + post-LN
    residual (C8, reference Decoder.py:7-42)."""

    def __init__(self, d_model, num_heads, dff, rate=0.1):
        super().__init__()
        self.mha1 = SelfAttention(d_model, num_heads)
        self.mha2 = CrossAttention(d_model, num_heads)
        self.ffn = FeedForward(d_model, dff)
        self.ln1 = _LN(d_model)
        self.ln2 = _LN(d_model)
        self.ln3 = _LN(d_model)
        self.rate = rate

    def forward(self, x, enc_output, tgt_pad, src_pad, training,
                return_weights=False, tgt_seg=None, src_seg=None):
        heads1, w1 = self.mha1(x, kv_pad=tgt_pad, causal=True,
                               return_weights=return_weights, project=False,
                               seg=tgt_seg)
        out1 = _proj_ln(self.mha1, heads1, x, self.ln1, self.rate, training)
        heads2, w2 = self.mha2(out1, enc_output, kv_pad=src_pad,
                               return_weights=return_weights, project=False,
                               q_seg=tgt_seg, kv_seg=src_seg)
        out2 = _proj_ln(self.mha2, heads2, out1, self.ln2, self.rate,
                        training)
        out3 = _ffn_ln(self.ffn, out2, self.ln3, self.rate, training)
        return out3, w1, w2


def _embed(tokens, weight, pe, positions):
    if positions is None:
        return ops.embedding_scale_pe(tokens, weight, pe)
    return ops.embedding_scale_pe(tokens, weight, pe, positions=positions)


class Encoder(nn.Module):
    """Embedding ×√d + PE + dropout -> L encoder layers (C7,
    reference Encoder.py:31-60)."""

    def __init__(self, num_layers, d_model, num_heads, dff, input_vocab_size,
                 rate=0.1, max_position=4096):
        super().__init__()
        self.d_model, self.num_layers = d_model, num_layers
        self.embedding = nn.Parameter(torch.empty(input_vocab_size, d_model)
                                      .uniform_(-0.05, 0.05))
        # PE table sized by max seq len, not vocab; concat
        # layout (Q2). Stored fp32, registered as a buffer (not a parameter).
        pe = R.positional_encoding(max_position, d_model).squeeze(0)
        self.register_buffer("pe", pe, persistent=False)
        self.layers = nn.ModuleList(
            EncoderLayer(d_model, num_heads, dff, rate) for _ in range(num_layers))
        self.rate = rate

    def forward(self, tokens, src_pad, training, seg=None, positions=None):
        x = _embed(tokens, self.embedding, self.pe, positions)
        x = ops.dropout(x, self.rate, training)
        for layer in self.layers:
            x = layer(x, src_pad, training, seg=seg)
        return x


class Decoder(nn.Module):
    """Embedding + PE -> L decoder layers; collects per-layer attention
    weights (keys 'decoder_layer{i}_block{1,2}', reference Decoder.py:75-76)
    only in inspection mode."""

    def __init__(self, num_layers, d_model, num_heads, dff, target_vocab_size,
                 rate=0.1, max_position=4096):
        super().__init__()
        self.d_model, self.num_layers = d_model, num_layers
        self.embedding = nn.Parameter(torch.empty(target_vocab_size, d_model)
                                      .uniform_(-0.05, 0.05))
        pe = R.positional_encoding(max_position, d_model).squeeze(0)
        self.register_buffer("pe", pe, persistent=False)
        self.layers = nn.ModuleList(
            DecoderLayer(d_model, num_heads, dff, rate) for _ in range(num_layers))
        self.rate = rate

    def forward(self, tokens, enc_output, tgt_pad, src_pad, training,
                return_weights=False, tgt_seg=None, src_seg=None,
                positions=None):
        x = _embed(tokens, self.embedding, self.pe, positions)
        x = ops.dropout(x, self.rate, training)
        attention_weights = {}
        for i, layer in enumerate(self.layers):
            x, w1, w2 = layer(x, enc_output, tgt_pad, src_pad, training,
                              return_weights=return_weights,
                              tgt_seg=tgt_seg, src_seg=src_seg)
            if return_weights:
                attention_weights[f"decoder_layer{i + 1}_block1"] = w1
                attention_weights[f"decoder_layer{i + 1}_block2"] = w2
        return x, attention_weights


class Transformer(nn.Module):
    """Top-level model (C10, reference Transformer.py:5-32).

    call((inp, tar), training) -> (logits, attention_weights) — the reference
    signature; attention_weights is {} unless return_weights=True (Q13).

    A packed input (data.PackedBatch, or anything with its src / src_seg /
    src_pos / tar_inp / tgt_seg / tgt_pos fields) holds several sentence
    pairs per row: attention is confined to each pair by the segment ids and
    the positional encoding restarts at every sentence, so each pair computes
    what it would compute in a row of its own.  Logits are (B, L, V) in the
    packed layout; tar_real of the same batch labels them."""

    def __init__(self, num_layers, d_model, num_heads, dff, input_vocab_size,
                 target_vocab_size, rate=0.1, max_position=4096):
        super().__init__()
        self.encoder = Encoder(num_layers, d_model, num_heads, dff,
                               input_vocab_size, rate, max_position)
        self.decoder = Decoder(num_layers, d_model, num_heads, dff,
                               target_vocab_size, rate, max_position)
        self.w_final = nn.Parameter(_glorot(target_vocab_size, d_model))
        self.b_final = nn.Parameter(torch.zeros(target_vocab_size))

    def _forward_packed(self, pb, training, return_weights):
        i32 = torch.int32   # converted ONCE; the per-layer wrappers no-op
        src_seg = pb.src_seg.to(i32).contiguous()
        tgt_seg = pb.tgt_seg.to(i32).contiguous()
        enc_output = self.encoder(pb.src, None, training, seg=src_seg,
                                  positions=pb.src_pos.to(i32).contiguous())
        dec_output, attention_weights = self.decoder(
            pb.tar_inp, enc_output, None, None, training, return_weights,
            tgt_seg=tgt_seg, src_seg=src_seg,
            positions=pb.tgt_pos.to(i32).contiguous())
        logits = ops.linear(dec_output, self.w_final, self.b_final)
        return logits, attention_weights

    def forward(self, inputs, training=False, return_weights=False):
        if hasattr(inputs, "src_seg"):
            return self._forward_packed(inputs, training, return_weights)
        inp, tar = inputs
        # mask construction (C5) folds into the attention kernels' predicate
        # logic: only per-token pad flags cross the boundary.
        # Converted to uint8 ONCE here — the per-layer kernel wrappers'
        # .to(uint8).contiguous() then no-op instead of copying per layer
        # (was 18 copy kernels/step).
        src_pad = (inp == 0).to(torch.uint8)
        tgt_pad = (tar == 0).to(torch.uint8)
        enc_output = self.encoder(inp, src_pad, training)
        dec_output, attention_weights = self.decoder(
            tar, enc_output, tgt_pad, src_pad, training, return_weights)
        logits = ops.linear(dec_output, self.w_final, self.b_final)
        return logits, attention_weights

    # convenience alias matching the reference's .call
    call = forward


# ---------------------------------------------------------------------------
# KV-cached incremental decoding (inference).  The reference's predict loop
# re-runs the FULL encoder + decoder prefix for every generated token
# (reference train.py:109-118); SURVEY.md §3.3 marks that as the naive
# contract, not a design to copy.  Here: the encoder runs once, each decoder
# layer keeps a packed (B, S_max, 2, H, dh) self-attention KV cache appended
# in place, and cross-attention K/V are projected from the encoder output
# once.  Each decode step costs O(1) in sequence length for the projections
# and O(t) for the cached attention reads.
# ---------------------------------------------------------------------------

class DecodeCache:
    """Per-layer packed KV caches + precomputed cross K/V."""

    def __init__(self, model: "Transformer", B: int, max_len: int,
                 enc_output: torch.Tensor, src_pad: torch.Tensor):
        dec = model.decoder
        d = dec.d_model
        layer0 = dec.layers[0]
        H, dh = layer0.mha1.num_heads, layer0.mha1.depth
        dev, dt = enc_output.device, enc_output.dtype
        self.pos = 0
        self.max_len = max_len
        self.enc_output = enc_output
        self.src_pad = src_pad
        self.self_kv = [torch.empty(B, max_len, 2, H, dh, device=dev, dtype=dt)
                        for _ in dec.layers]
        # cross K/V once per sequence (B, Sk, 2, H, dh)
        self.cross_kv = []
        Sk = enc_output.shape[1]
        for layer in dec.layers:
            kv = ops.linear(enc_output, layer.mha2.w_kv, layer.mha2.b_kv)
            self.cross_kv.append(kv.view(B, Sk, 2, H, dh))


@torch.no_grad()
def encode(model, inp, training=False):
    """Run the encoder once; returns (enc_output, src_pad)."""
    src_pad = (inp == 0).to(torch.uint8)
    return model.encoder(inp, src_pad, training), src_pad


@torch.no_grad()
def decode_step(model, tokens_new, cache: DecodeCache):
    """One incremental decoder step.

    tokens_new: (B, 1) int64 — the latest target token per sequence.
    Returns logits (B, 1, V) for the next-token distribution."""
    dec = model.decoder
    B = tokens_new.shape[0]
    t = cache.pos
    # embedding * sqrt(d) + PE at position t
    x = ops.embedding_scale_pe_at(tokens_new, dec.embedding, dec.pe, t)
    for li, layer in enumerate(dec.layers):
        H, dh = layer.mha1.num_heads, layer.mha1.depth
        # masked self-attention against the cache: project packed qkv for the
        # new row, append k/v in place, attend over positions [0, t].
        qkv = ops.linear(x, layer.mha1.w_qkv, layer.mha1.b_qkv)
        qkv = qkv.view(B, 1, 3, H, dh)
        cache.self_kv[li][:, t:t + 1] = qkv[:, :, 1:3]
        q = qkv[:, :, 0].contiguous()
        kv_hist = cache.self_kv[li][:, :t + 1]
        k, v = kv_hist.unbind(dim=2)
        attn1 = ops.fused_attention(q, k, v)  # all cached keys visible
        attn1 = ops.linear(attn1.reshape(B, 1, H * dh),
                           layer.mha1.w_o, layer.mha1.b_o)
        out1 = ops.residual_layernorm(attn1, x, layer.ln1.gamma,
                                      layer.ln1.beta, layer.ln1.eps)
        # cross-attention against precomputed encoder K/V
        q2 = ops.linear(out1, layer.mha2.w_q, layer.mha2.b_q)
        q2 = q2.view(B, 1, H, dh)
        k2, v2 = cache.cross_kv[li].unbind(dim=2)
        attn2 = ops.fused_attention(q2, k2, v2, kv_pad=cache.src_pad)
        attn2 = ops.linear(attn2.reshape(B, 1, H * dh),
                           layer.mha2.w_o, layer.mha2.b_o)
        out2 = ops.residual_layernorm(attn2, out1, layer.ln2.gamma,
                                      layer.ln2.beta, layer.ln2.eps)
        ffn = layer.ffn(out2)
        x = ops.residual_layernorm(ffn, out2, layer.ln3.gamma,
                                   layer.ln3.beta, layer.ln3.eps)
    cache.pos = t + 1
    return ops.linear(x, model.w_final, model.b_final)


@torch.no_grad()
def greedy_decode(model, inp, start_id, end_id, max_len=10):
    """KV-cached greedy decode.  inp (B, S) int64; returns (B, <=max_len+1)
    token ids starting with start_id; stops early when every sequence has
    emitted end_id."""
    B = inp.shape[0]
    enc_output, src_pad = encode(model, inp)
    cache = DecodeCache(model, B, max_len + 1, enc_output, src_pad)
    out = torch.full((B, 1), start_id, dtype=torch.int64, device=inp.device)
    finished = torch.zeros(B, dtype=torch.bool, device=inp.device)
    for _ in range(max_len):
        logits = decode_step(model, out[:, -1:], cache)
        nxt = ops.argmax_lastdim(logits).view(B, 1)
        out = torch.cat([out, nxt], dim=-1)
        finished |= (nxt.squeeze(1) == end_id)
        if bool(finished.all()):
            break
    # Rows that finished early kept receiving argmax tokens while other
    # rows decoded — mask them so batched output matches single-sentence
    # and GraphedDecoder output for the same sentence.
    return mask_after_end(out, end_id)


def mask_after_end(out: torch.Tensor, end_id: int) -> torch.Tensor:
    """Zero every token after the first end_id per row (in place)."""
    hit = (out == end_id).cumsum(dim=1) > 0
    mask = hit.roll(1, dims=1)
    mask[:, 0] = False
    out[mask] = 0
    return out


# ---------------------------------------------------------------------------
# hipGraph-captured decoding (serving): one replay per token.  The eager
# decode_step launches hundreds of tiny kernels per token (launch-bound at
# small batch, ~2.3 ms/token at B=1); here the whole step is captured once
# with a DEVICE position counter and replayed.  Fixed-size zero-initialized
# KV caches are attended with a pad mask that the captured step itself
# unmasks one slot per replay (index_fill_ on the device position), so no
# host work happens between tokens beyond the replay call.
# ---------------------------------------------------------------------------

class GraphedDecoder:
    """Captures one decoder step for fixed (B, src) shapes; __call__ decodes
    max_len tokens with one graph replay per token."""

    @torch.no_grad()
    def __init__(self, model: "Transformer", B: int, S_src: int, max_len: int,
                 start_id: int, device):
        assert max_len >= 4, "warmup+capture advance the position past 3"
        self.model = model
        self.B, self.S_src, self.max_len = B, S_src, max_len
        self.start_id = start_id
        dec = model.decoder
        layer0 = dec.layers[0]
        H, dh = layer0.mha1.num_heads, layer0.mha1.depth
        dt = next(model.parameters()).dtype
        self.inp = torch.zeros(B, S_src, dtype=torch.int64, device=device)
        self.enc_output = torch.zeros(B, S_src, dec.d_model, device=device,
                                      dtype=dt)
        self.src_pad = torch.zeros(B, S_src, dtype=torch.uint8, device=device)
        self.self_kv = [torch.zeros(B, max_len, 2, H, dh, device=device,
                                    dtype=dt) for _ in dec.layers]
        self.cross_kv = [torch.zeros(B, S_src, 2, H, dh, device=device,
                                     dtype=dt) for _ in dec.layers]
        self.kv_pad = torch.ones(B, max_len, dtype=torch.uint8, device=device)
        self.tok = torch.zeros(B, max_len + 1, dtype=torch.int64,
                               device=device)
        self.pos = torch.zeros(1, dtype=torch.int64, device=device)

        def step():
            from .. import ops as O
            pos = self.pos
            # this replay's cache slot becomes visible
            self.kv_pad.index_fill_(1, pos, 0)
            cur = self.tok.index_select(1, pos)            # (B,1)
            pe_row = dec.pe.index_select(0, pos)           # (1,d) model dtype
            # same kernel as the eager decode path -> bit-identical tokens
            x = O.ext().embed_pe_fwd(cur, dec.embedding, pe_row)
            for li, layer in enumerate(dec.layers):
                qkv = O.linear(x, layer.mha1.w_qkv, layer.mha1.b_qkv)
                qkv = qkv.view(B, 1, 3, H, dh)
                self.self_kv[li].index_copy_(1, pos, qkv[:, :, 1:3])
                q = qkv[:, :, 0].contiguous()
                k, v = self.self_kv[li].unbind(dim=2)
                attn1 = O.fused_attention(q, k, v, kv_pad=self.kv_pad)
                attn1 = O.linear(attn1.reshape(B, 1, H * dh),
                                 layer.mha1.w_o, layer.mha1.b_o)
                out1 = O.residual_layernorm(attn1, x, layer.ln1.gamma,
                                            layer.ln1.beta, layer.ln1.eps)
                q2 = O.linear(out1, layer.mha2.w_q, layer.mha2.b_q)
                q2 = q2.view(B, 1, H, dh)
                k2, v2 = self.cross_kv[li].unbind(dim=2)
                attn2 = O.fused_attention(q2, k2, v2, kv_pad=self.src_pad)
                attn2 = O.linear(attn2.reshape(B, 1, H * dh),
                                 layer.mha2.w_o, layer.mha2.b_o)
                out2 = O.residual_layernorm(attn2, out1, layer.ln2.gamma,
                                            layer.ln2.beta, layer.ln2.eps)
                ffn = layer.ffn(out2)
                x = O.residual_layernorm(ffn, out2, layer.ln3.gamma,
                                         layer.ln3.beta, layer.ln3.eps)
            logits = O.linear(x, self.model.w_final, self.model.b_final)
            nxt = O.argmax_lastdim(logits).view(B, 1)
            self.tok.index_copy_(1, pos + 1, nxt)
            self.pos.add_(1)

        # warmup on a side stream, then capture.  capture hint: library
        # GEMM kernels inside the graph (launch cost is replayed away).
        from ..ops.functional import set_capture_hint
        set_capture_hint(True)
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                step()
                step()
            torch.cuda.current_stream().wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph):
                step()
        finally:
            set_capture_hint(False)

    @torch.no_grad()
    def __call__(self, inp: torch.Tensor, end_id: int,
                 max_len: int | None = None) -> torch.Tensor:
        """inp (B, S_src) int64 -> (B, n+1) ids starting with start_id;
        tokens after the first end_id per row are zeroed."""
        n = min(max_len or self.max_len, self.max_len)
        assert inp.shape == (self.B, self.S_src), (inp.shape, self.B)
        self.inp.copy_(inp)
        enc, src_pad = encode(self.model, self.inp)
        self.enc_output.copy_(enc)
        self.src_pad.copy_(src_pad.to(torch.uint8))
        dec = self.model.decoder
        for li, layer in enumerate(dec.layers):
            kv = ops.linear(self.enc_output, layer.mha2.w_kv, layer.mha2.b_kv)
            self.cross_kv[li].copy_(
                kv.view(self.B, self.S_src, 2, layer.mha2.num_heads,
                        layer.mha2.depth))
        self.kv_pad.fill_(1)
        self.self_kv and [t.zero_() for t in self.self_kv]
        self.tok.zero_()
        self.tok[:, 0] = self.start_id
        self.pos.zero_()
        for _ in range(n):
            self.graph.replay()
        out = self.tok[:, :n + 1].clone()
        # zero everything after the first end_id per row (parity with the
        # early-stopping eager decode)
        return mask_after_end(out, end_id)
