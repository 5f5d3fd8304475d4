"""Autograd-integrated op layer with device dispatch.

GPU (CUDA/ROCm) tensors run via `torch.autograd.Function` wrappers
(SURVEY.md §2.3), and — since round 2 — EVERY training-shape op runs a
hand-written CDNA4 HIP kernel, GEMMs included: forwards on the
gemm256/gemm128 NT dispatch, dX against a per-step cached transposed
weight (ONE batched-transpose launch/step), the d_model dW shapes on the
split-contraction tr16 kernel and the wide logits dW on the TRxTR
gemm_uni kernel.  Every dispatch choice is measured per shape
(docs/PERF.md round 2); hipBLASLt survives only as the
TFMX_FWD_GEMM=blaslt / TFMX_DX=blaslt A/B arms.  CPU tensors run the
fp32 reference math in reference.py through plain differentiable torch
ops.  The GPU path never falls back silently: if the extension is
missing it raises (see ops/__init__.py).
"""

from __future__ import annotations

import math

import torch

from . import reference as R
from . import ext
from .gemm_dispatch import (  # noqa: F401  (re-exported: graph.py, optimizer,
    bump_weight_version,      # models and tests reach for them here)
    prepare_weight_caches,
    refresh_weight_caches,
    set_capture_hint,
    _dense2d,
    _dw_db_gemm,
    _dw_gemm,
    _dx_epilogue_ok,
    _dx_gemm,
    _fwd_gemm,
    _wt_padded,
)


# ---------------------------------------------------------------------------
# Flat-gradient fast path.  When a parameter carries a `_flat_grad` view
# (runtime/optimizer.py FlatParams), the op wrappers below hide it from
# autograd entirely: the backward kernel writes the weight gradient straight
# into the flat buffer slice (no per-parameter AccumulateGrad kernel, no
# clone — autograd ALWAYS clones view gradients, so returning the view would
# cost an extra copy per parameter per step).  The DP bucket manager
# subscribes here for gradient-readiness instead of post-accumulate hooks.
# ---------------------------------------------------------------------------

def set_grad_ready_callback(params, fn):
    """fn(param) is invoked (backward order) right after a parameter's
    gradient kernels are enqueued on the compute stream.  Used by
    parallel/ddp.py to launch bucket all-reduces.  Registration is scoped
    to the given parameters (not process-global): a second
    BucketedDataParallel over a different model cannot hijack the first,
    and fn=None unregisters."""
    for p in params:
        if fn is None:
            if hasattr(p, "_grad_ready_cb"):
                del p._grad_ready_cb
        else:
            p._grad_ready_cb = fn


def _grad_ready(*params):
    for p in params:
        if p is not None:
            cb = getattr(p, "_grad_ready_cb", None)
            if cb is not None:
                cb(p)


def _flat(p):
    return getattr(p, "_flat_grad", None) if p is not None else None


# Each autograd Function below has ONE body for both modes.  Its parameter
# slots hold the tensors in autograd mode and None in flat mode, where the
# parameters travel in the `hidden` list instead (a list is opaque to
# autograd, so only the activations are differentiable).  backward hands
# every gradient kernel its destination from _grad_dst, then in flat mode
# fires _grad_ready and returns None in the parameter slots.

def _slots(flat, *params):
    """The (*parameter slots, hidden) arguments of apply()."""
    if flat:
        return (None,) * len(params) + (list(params),)
    return params + (None,)


def _grad_dst(p, flat):
    """Where the backward kernel writes parameter `p`'s gradient: p's slice
    of the flat buffer (a matrix as 2-D rows, a vector 1-D), or a fresh
    tensor that backward hands back to autograd."""
    if p is None:
        return None
    if not flat:
        return torch.empty_like(p)
    fg = p._flat_grad
    return fg.view(p.shape[0], -1) if p.dim() > 1 else fg.view(-1)


# ---------------------------------------------------------------------------
# Dropout seeds (K11): from the torch RNG, or from a device counter under
# HIP-graph capture.  While a step is being captured the
# seed must come from a DEVICE counter (advanced in-graph by the optimizer's
# adam_coefs kernel) — a host seed would be baked into the graph and every
# replay would reuse the same mask.  Each call site gets a distinct salt
# (capture order is deterministic).
# ---------------------------------------------------------------------------

_GRAPH_SEED_T = None
_GRAPH_SALT = [0]


def set_graph_rng(seed_tensor):
    """Install (or clear, with None) the device seed tensor used by dropout
    during graph capture."""
    global _GRAPH_SEED_T
    _GRAPH_SEED_T = seed_tensor
    _GRAPH_SALT[0] = 0


def _dropout_seed():
    """The trailing (seed, seed_t) arguments of E.ln_fwd / E.dropout_fwd for
    ONE dropout site: the next salt plus the device seed tensor under graph
    capture, otherwise one host draw from the torch RNG."""
    if _GRAPH_SEED_T is not None:
        _GRAPH_SALT[0] += 1
        return _GRAPH_SALT[0], _GRAPH_SEED_T
    return int(torch.randint(0, 2**31 - 1, (1,)).item()), None


# ---------------------------------------------------------------------------
# Linear: y = x @ W^T + b, optional fused ReLU epilogue (K1/K7/K8/K12).
# Backend choice per GEMM: gemm_dispatch.py.
# ---------------------------------------------------------------------------

class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, hidden, activation):
        # x: (M, K) bf16; w: (N, K) bf16; b: (N,) bf16 or None
        E = ext()
        ctx.flat = hidden is not None
        if ctx.flat:
            w, b = hidden
        y = _fwd_gemm(E, x, w, b, activation)
        ctx.activation = activation
        ctx.params = (w, b)
        ctx.save_for_backward(x, y if activation == "relu" else torch.Tensor())
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        x, y = ctx.saved_tensors
        w, b = ctx.params
        flat = ctx.flat
        db = None
        if ctx.activation == "relu" and b is not None:
            # dz = dy * (y > 0) and db = colsum(dz) in one row-streaming
            # pass: the kernel that writes dz carries its column sums, so
            # dz is not read a second time for the bias gradient.
            dy, db = E.relu_bwd_db(dy.contiguous(), y, _grad_dst(b, flat))
        elif ctx.activation == "relu":
            dy = E.relu_bwd(dy.contiguous(), y)  # dz = dy * (y > 0)
        else:
            dy = _dense2d(dy)
        dx = _dx_gemm(E, dy, w)         # dX[M,K] = dY[M,N] @ W[N,K]
        dw, db = _dw_db_gemm(dy, x, b is not None, w_out=_grad_dst(w, flat),
                             b_out=_grad_dst(b, flat), db=db)
        if flat:
            _grad_ready(w, b)
            dw = db = None
        return dx, dw, db, None, None


def linear(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None = None,
           activation: str | None = None) -> torch.Tensor:
    """y = x @ W^T + b (+ReLU). x may have leading batch dims."""
    if x.is_cuda:
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        y = _LinearFn.apply(x2, *_slots(_flat(w) is not None, w, b),
                            activation)
        return y.view(*shp[:-1], w.shape[0])
    y = torch.nn.functional.linear(x, w, b)
    if activation == "relu":
        y = torch.relu(y)
    return y


# ---------------------------------------------------------------------------
# Fused flash-style attention (K2-K5, K14). Layout (B, S, H, dh) throughout —
# the head split/merge transposes of reference Attention.py:52-57,74-76 are
# eliminated.
# ---------------------------------------------------------------------------

def _attn_fwd(E, q, k, v, kv_pad, q_seg, kv_seg, causal, scale):
    """Forward kernel: the segment instantiation when ids are given (kv_pad
    is then unused: id 0 is the padding), else today's call unchanged."""
    if q_seg is not None:
        return E.attn_fwd_seg(q, k, v, q_seg, kv_seg, causal, scale)
    return E.attn_fwd(q, k, v,
                      kv_pad if kv_pad is not None else torch.Tensor(),
                      causal, scale)


def _attn_bwd(E, q, k, v, o, do, lse, kv_pad, q_seg, kv_seg, causal, scale,
              mode):
    if q_seg.numel():
        return E.attn_bwd_seg(q, k, v, o, do, lse, q_seg, kv_seg, causal,
                              scale, mode)
    return E.attn_bwd(q, k, v, o, do, lse, kv_pad, causal, scale, mode)


def _opt(t):
    return t if t is not None else torch.Tensor()


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, kv_pad, causal, scale, q_seg=None,
                kv_seg=None):
        E = ext()
        o, lse = _attn_fwd(E, q, k, v, kv_pad, q_seg, kv_seg, causal, scale)
        ctx.causal = causal
        ctx.scale = scale
        ctx.save_for_backward(q, k, v, o, lse, _opt(kv_pad), _opt(q_seg),
                              _opt(kv_seg))
        return o

    @staticmethod
    def backward(ctx, do):
        E = ext()
        q, k, v, o, lse, kv_pad, q_seg, kv_seg = ctx.saved_tensors
        dq, dk, dv = _attn_bwd(E, q, k, v, o, do.contiguous(), lse, kv_pad,
                               q_seg, kv_seg, ctx.causal, ctx.scale, 0)
        return dq, dk, dv, None, None, None, None, None


class _SelfAttnPackedFn(torch.autograd.Function):
    """Attention straight on the packed (B,S,3,H,dh) QKV tensor: the kernels
    read the q/k/v slots through strides (no contiguous copies) and backward
    writes one packed dQKV (no cat/stack kernels)."""

    @staticmethod
    def forward(ctx, qkv, kv_pad, causal, scale, seg=None):
        E = ext()
        q, k, v = qkv.unbind(dim=2)  # strided views, never materialized
        o, lse = _attn_fwd(E, q, k, v, kv_pad, seg, seg, causal, scale)
        ctx.causal = causal
        ctx.scale = scale
        ctx.save_for_backward(qkv, o, lse, _opt(kv_pad), _opt(seg))
        return o

    @staticmethod
    def backward(ctx, do):
        E = ext()
        qkv, o, lse, kv_pad, seg = ctx.saved_tensors
        q, k, v = qkv.unbind(dim=2)
        (dqkv,) = _attn_bwd(E, q, k, v, o, do.contiguous(), lse, kv_pad,
                            seg, seg, ctx.causal, ctx.scale, 1)
        return dqkv, None, None, None, None


class _CrossAttnPackedFn(torch.autograd.Function):
    """Cross attention: q (B,Sq,H,dh) + packed kv (B,Sk,2,H,dh)."""

    @staticmethod
    def forward(ctx, q, kv, kv_pad, scale, q_seg=None, kv_seg=None):
        E = ext()
        k, v = kv.unbind(dim=2)
        o, lse = _attn_fwd(E, q, k, v, kv_pad, q_seg, kv_seg, False, scale)
        ctx.scale = scale
        ctx.save_for_backward(q, kv, o, lse, _opt(kv_pad), _opt(q_seg),
                              _opt(kv_seg))
        return o

    @staticmethod
    def backward(ctx, do):
        E = ext()
        q, kv, o, lse, kv_pad, q_seg, kv_seg = ctx.saved_tensors
        k, v = kv.unbind(dim=2)
        dq, dkv = _attn_bwd(E, q, k, v, o, do.contiguous(), lse, kv_pad,
                            q_seg, kv_seg, False, ctx.scale, 2)
        return dq, dkv, None, None, None, None


def _seg_ids(q_seg, kv_seg):
    """Both or neither; int32 contiguous for the kernels."""
    if (q_seg is None) != (kv_seg is None):
        raise ValueError("q_seg and kv_seg must be given together")
    if q_seg is None:
        return None, None
    return (q_seg.to(torch.int32).contiguous(),
            kv_seg.to(torch.int32).contiguous())


def self_attention(qkv, kv_pad=None, causal=False, return_weights=False,
                   q_seg=None, kv_seg=None):
    """qkv: (B,S,3,H,dh).  GPU path never materializes q/k/v copies.
    q_seg/kv_seg: (B,S) segment ids of a packed row (see fused_attention);
    self-attention passes the same array for both."""
    B, S, _, H, dh = qkv.shape
    scale = 1.0 / math.sqrt(dh)
    if qkv.is_cuda and not return_weights:
        if q_seg is not None:
            if kv_seg is not q_seg and not torch.equal(q_seg, kv_seg):
                raise ValueError("self_attention needs q_seg == kv_seg")
            seg, _ = _seg_ids(q_seg, q_seg)
            return _SelfAttnPackedFn.apply(qkv, None, causal, scale, seg)
        kp = kv_pad.to(torch.uint8).contiguous() if kv_pad is not None else None
        return _SelfAttnPackedFn.apply(qkv, kp, causal, scale)
    q, k, v = qkv.unbind(dim=2)
    return fused_attention(q, k, v, kv_pad=kv_pad, causal=causal,
                           return_weights=return_weights, q_seg=q_seg,
                           kv_seg=kv_seg)


def cross_attention(q, kv, kv_pad=None, return_weights=False, q_seg=None,
                    kv_seg=None):
    """q: (B,Sq,H,dh); kv: (B,Sk,2,H,dh).  q_seg (B,Sq) / kv_seg (B,Sk):
    target / source segment ids of a packed row; pair n is id n on both."""
    dh = q.shape[-1]
    scale = 1.0 / math.sqrt(dh)
    if q.is_cuda and not return_weights:
        if q_seg is not None or kv_seg is not None:
            qs, ks = _seg_ids(q_seg, kv_seg)
            return _CrossAttnPackedFn.apply(q.contiguous(), kv, None, scale,
                                            qs, ks)
        kp = kv_pad.to(torch.uint8).contiguous() if kv_pad is not None else None
        return _CrossAttnPackedFn.apply(q.contiguous(), kv, kp, scale)
    k, v = kv.unbind(dim=2)
    return fused_attention(q, k, v, kv_pad=kv_pad, causal=False,
                           return_weights=return_weights, q_seg=q_seg,
                           kv_seg=kv_seg)


def fused_attention(q, k, v, kv_pad=None, causal=False, return_weights=False,
                    q_seg=None, kv_seg=None):
    """q: (B,Sq,H,dh), k/v: (B,Sk,H,dh); kv_pad: (B,Sk) bool/uint8, True=pad.

    Masking semantics match reference Attention.py:25-26: masked logits get
    -1e9 added before softmax. Returns (B,Sq,H,dh); attention weights only on
    the eager/inspection path.

    q_seg (B,Sq) / kv_seg (B,Sk): integer segment ids of packed rows (1,2,..
    contiguous in order, 0 = padding, zeros only at the tail).  A query sees
    exactly the keys of its own non-zero id (and, under `causal`, those at or
    before it); kv_pad is then ignored.  Hidden keys get weight exactly 0,
    and an id-0 query row yields a zero output row and zero gradients — not
    the additive rule's uniform attention."""
    scale = 1.0 / math.sqrt(q.shape[-1])
    if (q_seg is None) != (kv_seg is None):
        raise ValueError("q_seg and kv_seg must be given together")
    if q.is_cuda and not return_weights:
        if q_seg is not None:
            qs, ks = _seg_ids(q_seg, kv_seg)
            return _AttentionFn.apply(q.contiguous(), k.contiguous(),
                                      v.contiguous(), None, causal, scale,
                                      qs, ks)
        kp = kv_pad.to(torch.uint8).contiguous() if kv_pad is not None else None
        return _AttentionFn.apply(q.contiguous(), k.contiguous(), v.contiguous(),
                                  kp, causal, scale)
    # eager path (CPU, or weight inspection): (B,S,H,dh) -> (B,H,S,dh)
    qt, kt, vt = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    mask = None
    B, Sq, H, _ = q.shape
    Sk = k.shape[1]
    if q_seg is not None:
        # the equivalent dense mask; fp32 exp(-1e9 - max) is exactly 0, so
        # visible rows match the kernels' selection, and id-0 query rows
        # (uniform under the additive rule) are zeroed below
        assert not causal or Sq == Sk, "causal attention requires Sq == Sk"
        mask = R.create_segment_mask(q_seg, kv_seg, causal)
    else:
        if kv_pad is not None:
            mask = kv_pad.to(torch.float32)[:, None, None, :]
        if causal:
            la = R.create_look_ahead_mask(Sq, device=q.device)
            assert Sq == Sk, "causal attention requires Sq == Sk"
            mask = la[None, None] if mask is None else torch.maximum(mask, la[None, None])
    if q.dtype in (torch.bfloat16, torch.float16):
        qt, kt, vt = qt.float(), kt.float(), vt.float()
    out, w = R.scaled_dot_product_attention(qt, kt, vt, mask,
                                            return_weights=True)
    if q_seg is not None:
        live = (q_seg != 0)[:, None, :, None]
        out = out * live.to(out.dtype)
        w = w * live.to(w.dtype)
    out = out.permute(0, 2, 1, 3).to(q.dtype)
    if return_weights:
        return out, w
    return out


# ---------------------------------------------------------------------------
# Fused (dropout +) residual-add + LayerNorm, eps=1e-6 (K9), alone and as
# the tail of the sublayer composites: LN(dropout(linear(x)) + res) and the
# whole FFN block as ONE autograd node each.  The composites' forward runs
# the same kernels as the separate ops (same dropout-seed draws, same
# order).  Backward starts from the one-pass ln_bwd, which already streams
# dxm — the dY of the linear — and so delivers that linear's bias gradient
# for free (no colsum re-read); the FFN block can additionally apply the
# ReLU mask and the residual-branch add in the two dX GEMM epilogues
# (TFMX_FFN_BWD=fused, default off).
# ---------------------------------------------------------------------------

def _ln_drop_fwd(E, a, res, gamma, beta, eps, p):
    """(y, s, mean, rstd, mask) of LN(dropout(a) + res); p == 0 is the
    plain residual LN: no seed drawn, mask None."""
    if p > 0.0:
        return E.ln_fwd(a, res, gamma, beta, eps, p, *_dropout_seed())
    return (*E.ln_fwd(a, res, gamma, beta, eps), None)


def _ln_drop_bwd(E, ctx, dy, s, mean, rstd, mask, g, bt, b=None):
    """Fused ln_bwd writing dgamma/dbeta (and the bias gradient db of the
    linear feeding the dropout) to their destinations.
    Returns (dres, dxm, dgamma, dbeta, db); without dropout dxm is dres."""
    flat = ctx.flat
    dg, dbt, db = _grad_dst(g, flat), _grad_dst(bt, flat), _grad_dst(b, flat)
    out = E.ln_bwd(dy.contiguous(), s, g, mean, rstd, dg, dbt, mask, ctx.p,
                   db)
    if flat:
        _grad_ready(g, bt)
    return out[0], out[3] if mask is not None else out[0], dg, dbt, db


class _ResidualLNFn(torch.autograd.Function):
    """y = LN(dropout(x) + res): the sublayer dropout fused into the LN
    kernels — no standalone dropout read/write of the (B,S,d) tensor in
    either direction.  p = 0: y = LN(x + res)."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, hidden, p, eps):
        E = ext()
        ctx.flat = hidden is not None
        if ctx.flat:
            gamma, beta = hidden
        y, s, mean, rstd, mask = _ln_drop_fwd(E, x, res, gamma, beta, eps, p)
        ctx.p = p
        ctx.params = (gamma, beta)
        ctx.save_for_backward(s, mean, rstd, mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        s, mean, rstd, mask = ctx.saved_tensors
        g, bt = ctx.params
        # without dropout d/dx and d/dres are identical (y = LN(x + res))
        dres, dxm, dg, dbt, _ = _ln_drop_bwd(E, ctx, dy, s, mean, rstd, mask,
                                             g, bt)
        if ctx.flat:
            dg = dbt = None
        return dxm, dres, dg, dbt, None, None, None


class _LinearDropLNFn(torch.autograd.Function):
    """y = LN(dropout(x @ W^T + b) + res)."""

    @staticmethod
    def forward(ctx, x, res, w, b, gamma, beta, hidden, p, eps):
        E = ext()
        ctx.flat = hidden is not None
        if ctx.flat:
            w, b, gamma, beta = hidden
        a = _fwd_gemm(E, x, w, b, None)
        y, s, mean, rstd, mask = _ln_drop_fwd(E, a, res, gamma, beta, eps, p)
        ctx.p = p
        ctx.params = (w, b, gamma, beta)
        ctx.save_for_backward(x, s, mean, rstd, mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        x, s, mean, rstd, mask = ctx.saved_tensors
        w, b, g, bt = ctx.params
        flat = ctx.flat
        dres, dxm, dg, dbt, db = _ln_drop_bwd(E, ctx, dy, s, mean, rstd, mask,
                                              g, bt, b)
        dx = _dx_gemm(E, dxm, w)
        dw = _dw_gemm(dxm, x, out=_grad_dst(w, flat))
        if flat:
            _grad_ready(w, b)
            dw = db = dg = dbt = None
        return dx, dres, dw, db, dg, dbt, None, None, None


class _FFNDropLNFn(torch.autograd.Function):
    """y = LN(dropout(relu(x @ W1^T + b1) @ W2^T + b2) + x)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, hidden, p, eps):
        E = ext()
        ctx.flat = hidden is not None
        if ctx.flat:
            w1, b1, w2, b2, gamma, beta = hidden
        h = _fwd_gemm(E, x, w1, b1, "relu")
        a = _fwd_gemm(E, h, w2, b2, None)
        y, s, mean, rstd, mask = _ln_drop_fwd(E, a, x, gamma, beta, eps, p)
        ctx.p = p
        ctx.params = (w1, b1, w2, b2, gamma, beta)
        ctx.save_for_backward(x, h, s, mean, rstd, mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        # _grad_ready order (DDP overlap): (g, bt), then (w2, b2) before
        # the dZ GEMM, then (w1, b1) before the final dX.
        E = ext()
        x, h, s, mean, rstd, mask = ctx.saved_tensors
        w1, b1, w2, b2, g, bt = ctx.params
        flat = ctx.flat
        dres, dxm, dg, dbt, db2 = _ln_drop_bwd(E, ctx, dy, s, mean, rstd,
                                               mask, g, bt, b2)
        dw2 = _dw_gemm(dxm, h, out=_grad_dst(w2, flat))
        if flat:
            _grad_ready(w2, b2)
        M, d, dff = x.shape[0], x.shape[1], h.shape[1]
        nob = torch.Tensor()
        if _dx_epilogue_ok(E, M, dff, d):
            # dz = (dxm @ W2) * (h > 0), mask applied on the accumulators
            dz = E.gemm256_nt(dxm, _wt_padded(E, w2), nob, 2, None, h)
            db1 = E.colsum(dz, _grad_dst(b1, flat)) if b1 is not None \
                else None
        elif b1 is not None:
            # the pass that writes dz also sums it: no colsum re-read
            dz, db1 = E.relu_bwd_db(_dx_gemm(E, dxm, w2).contiguous(), h,
                                    _grad_dst(b1, flat))
        else:
            dz = E.relu_bwd(_dx_gemm(E, dxm, w2).contiguous(), h)
            db1 = None
        dw1 = _dw_gemm(dz, x, out=_grad_dst(w1, flat))
        if flat:
            _grad_ready(w1, b1)
            dw1 = db1 = dw2 = db2 = dg = dbt = None
        if _dx_epilogue_ok(E, M, d, dff):
            # dx = dz @ W1 + dres in one rounding
            dx = E.gemm256_nt(dz, _wt_padded(E, w1), nob, 3, None, dres)
        else:
            dx = _dx_gemm(E, dz, w1) + dres
        return dx, dw1, db1, dw2, db2, dg, dbt, None, None, None


def _all_flat(*params):
    fl = [_flat(p) is not None for p in params if p is not None]
    return all(fl), any(fl)


def _rows(t):
    return t.reshape(-1, t.shape[-1]).contiguous()


def linear_dropout_residual_layernorm(x, w, b, res, gamma, beta, rate: float,
                                      training: bool, eps: float = 1e-6):
    """LN(dropout(x @ W^T + b) + res) — an attention block's output
    projection together with its post-sublayer dropout + residual LN.  One
    autograd node on GPU when training with rate > 0; otherwise (CPU, eval,
    rate 0, or only some parameters flat) the two separate ops."""
    allf, anyf = _all_flat(w, b, gamma, beta)
    if not (x.is_cuda and training and rate > 0.0 and allf == anyf):
        return dropout_residual_layernorm(linear(x, w, b), res, gamma, beta,
                                          rate, training, eps)
    y = _LinearDropLNFn.apply(_rows(x), _rows(res),
                              *_slots(allf, w, b, gamma, beta), rate, eps)
    return y.view(res.shape)


def ffn_dropout_residual_layernorm(x, w1, b1, w2, b2, gamma, beta,
                                   rate: float, training: bool,
                                   eps: float = 1e-6):
    """LN(dropout(relu(x @ W1^T + b1) @ W2^T + b2) + x) — the whole
    position-wise FFN sublayer; same fallback rule as above."""
    allf, anyf = _all_flat(w1, b1, w2, b2, gamma, beta)
    if not (x.is_cuda and training and rate > 0.0 and allf == anyf):
        h = linear(x, w1, b1, activation="relu")
        return dropout_residual_layernorm(linear(h, w2, b2), x, gamma, beta,
                                          rate, training, eps)
    y = _FFNDropLNFn.apply(_rows(x), *_slots(allf, w1, b1, w2, b2, gamma,
                                             beta), rate, eps)
    return y.view(x.shape)


def _residual_ln_gpu(x, res, gamma, beta, rate, eps):
    y = _ResidualLNFn.apply(_rows(x), _rows(res),
                            *_slots(_flat(gamma) is not None, gamma, beta),
                            rate, eps)
    return y.view(x.shape)


def residual_layernorm(x, res, gamma, beta, eps: float = 1e-6):
    if x.is_cuda:
        return _residual_ln_gpu(x, res, gamma, beta, 0.0, eps)
    if x.dtype in (torch.bfloat16, torch.float16):
        return R.residual_layernorm(x.float(), res.float(), gamma.float(),
                                    beta.float(), eps).to(x.dtype)
    return R.residual_layernorm(x, res, gamma, beta, eps)


def dropout_residual_layernorm(x, res, gamma, beta, rate: float,
                               training: bool, eps: float = 1e-6):
    """LN(dropout(x) + res) — the post-sublayer pattern of every encoder/
    decoder sublayer (reference Encoder.py:22-23).  Fused on GPU when
    training with rate>0; otherwise plain residual+LN / composed ops."""
    if not training or rate == 0.0:
        return residual_layernorm(x, res, gamma, beta, eps)
    if x.is_cuda:
        return _residual_ln_gpu(x, res, gamma, beta, rate, eps)
    xd = torch.nn.functional.dropout(x, p=rate, training=True)
    return residual_layernorm(xd, res, gamma, beta, eps)


# ---------------------------------------------------------------------------
# Fused embedding * sqrt(d) + positional encoding (K10).
# ---------------------------------------------------------------------------

class _EmbedPEFn(torch.autograd.Function):
    """Flat mode: the dW scatter-add casts straight into the flat view, and
    the weight slot holds a dummy differentiable `marker` instead — the
    output must still require grad (x flows onward), so something has to
    thread the graph."""

    @staticmethod
    def forward(ctx, tokens, weight, hidden, pe, positions=None):
        E = ext()
        ctx.flat = hidden is not None
        if ctx.flat:
            (weight,) = hidden
        if positions is not None:
            y = E.embed_pe_fwd(tokens, weight, pe, positions)
        else:
            y = E.embed_pe_fwd(tokens, weight, pe)
        ctx.weight = weight
        ctx.save_for_backward(tokens)
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        (tokens,) = ctx.saved_tensors
        weight = ctx.weight
        dw = E.embed_pe_bwd(dy.contiguous(), tokens, weight.shape[0],
                            _grad_dst(weight, ctx.flat))
        if ctx.flat:
            _grad_ready(weight)
            dw = None
        return None, dw, None, None, None


def embedding_scale_pe_at(tokens, weight, pe, pos: int):
    """Embedding + PE for an incremental decode step: positions start at
    `pos` instead of 0 (KV-cache path)."""
    return embedding_scale_pe(tokens, weight,
                              pe[pos:pos + tokens.shape[1]].contiguous())


def embedding_scale_pe(tokens, weight, pe, positions=None):
    """tokens (B,S) int; weight (V,d); pe (P,d) fp32 table, P >= S.
    positions (B,S) int, optional: the PE row of each token (packed rows,
    where the position restarts at every sentence) instead of its column."""
    if weight.is_cuda:
        extra = ()
        if positions is not None:
            extra = (positions.to(torch.int32).contiguous(),)
        if _flat(weight) is not None and torch.is_grad_enabled():
            marker = torch.empty(0, device=weight.device,
                                 dtype=weight.dtype, requires_grad=True)
            return _EmbedPEFn.apply(tokens.contiguous(), marker, [weight], pe,
                                    *extra)
        return _EmbedPEFn.apply(tokens.contiguous(), weight, None, pe, *extra)
    if weight.dtype in (torch.bfloat16, torch.float16):
        return R.embedding_scale_pe(tokens, weight.float(), pe[None].float(),
                                    positions).to(weight.dtype)
    return R.embedding_scale_pe(tokens, weight, pe[None].to(weight.dtype),
                                positions)


# ---------------------------------------------------------------------------
# Dropout (K11): mask saved for exact backward.
# ---------------------------------------------------------------------------

class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        y, mask = ext().dropout_fwd(x, p, *_dropout_seed())
        ctx.p = p
        ctx.save_for_backward(mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        (mask,) = ctx.saved_tensors
        return E.dropout_bwd(dy.contiguous(), mask, ctx.p), None


def dropout(x, p: float, training: bool):
    if not training or p == 0.0:
        return x
    if x.is_cuda:
        shp = x.shape
        return _DropoutFn.apply(x.reshape(-1).contiguous(), p).view(shp)
    return torch.nn.functional.dropout(x, p=p, training=True)


# ---------------------------------------------------------------------------
# Fused padding-masked (label-smoothed) cross entropy (K13).
# ---------------------------------------------------------------------------

class _CrossEntropyFn(torch.autograd.Function):
    """Loss AND gradient in ONE kernel at forward time (the gradient
    sweep re-reads rows that are still L2-hot, saving ce_bwd's separate
    full logits pass); the autograd seed is applied in backward by a
    device-side kernel that NO-OPS when the seed is 1.0 — the value
    loss.backward() always feeds — so numerics are exact for any seed
    without a host sync.  Memory is neutral: dfull (R, Vp) is saved
    instead of (logits, lse)."""

    @staticmethod
    def forward(ctx, logits, targets, batch_size, label_smoothing):
        E = ext()
        loss, dfull = E.ce_fused(logits, targets, float(batch_size),
                                 label_smoothing)
        ctx.V = logits.shape[1]
        ctx.save_for_backward(dfull)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        E = ext()
        (dfull,) = ctx.saved_tensors
        E.ce_scale(dfull, dloss.to(torch.float32).reshape(1).contiguous())
        # dfull is (R, Vp), Vp = roundup(V, 256), zero pad columns; the
        # [:, :V] view keeps the padded stride so the logits dX/dW GEMMs
        # contract over the aligned Vp (gemm_uni.hip)
        dlogits = dfull if dfull.shape[1] == ctx.V else dfull[:, :ctx.V]
        return dlogits, None, None, None


def masked_cross_entropy(logits, targets, batch_size, label_smoothing=0.0):
    """sum(CE * pad_mask)/batch_size (reference train.py:83-88)."""
    if logits.is_cuda:
        B, T, V = logits.shape
        return _CrossEntropyFn.apply(logits.reshape(-1, V).contiguous(),
                                     targets.reshape(-1).contiguous(),
                                     batch_size, label_smoothing)
    return R.masked_cross_entropy(logits, targets, batch_size, label_smoothing)


# ---------------------------------------------------------------------------
# Metrics / decode kernels (K16, K17).
# ---------------------------------------------------------------------------

def argmax_lastdim(logits):
    if logits.is_cuda:
        shp = logits.shape
        return ext().argmax_lastdim(logits.reshape(-1, shp[-1]).contiguous()).view(shp[:-1])
    return logits.argmax(dim=-1)


def masked_accuracy(logits, targets):
    correct, total = masked_accuracy_counts(logits, targets)
    return correct / max(total, 1)


def masked_accuracy_counts(logits, targets):
    """(correct, total) over non-pad target positions — lets callers
    accumulate token-weighted accuracy (the reference's streaming
    SparseCategoricalAccuracy semantics, train.py:72-73) instead of a
    mean of batch-means."""
    if logits.is_cuda:
        V = logits.shape[-1]
        correct, total = ext().accuracy(logits.reshape(-1, V).contiguous(),
                                        targets.reshape(-1).contiguous())
        return float(correct), float(total)
    pred = logits.argmax(dim=-1)
    mask = targets != 0
    return (float(((pred == targets) & mask).sum()), float(mask.sum()))


def masked_accuracy_counts_t(logits, targets):
    """[correct, total] as a float64 tensor on the logits' device, with NO
    host synchronisation (masked_accuracy_counts copies its two counters to
    the host on every call).  For callers that sum the counts of several
    micro-batches, or record them in a captured graph, and read them once."""
    pred = argmax_lastdim(logits)
    mask = targets != 0
    return torch.stack([((pred == targets) & mask).sum(),
                        mask.sum()]).to(torch.float64)
