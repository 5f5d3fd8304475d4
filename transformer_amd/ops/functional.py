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

import os

import torch

from . import reference as R
from . import ext


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


# ---------------------------------------------------------------------------
# Linear: y = x @ W^T + b, optional fused ReLU epilogue (K1/K7/K8/K12).
# ---------------------------------------------------------------------------


# GEMM backend (round 2): every training-shape GEMM runs hand-written.
# Forward goes to the gemm256/128 NT dispatch (measured best hand path:
# 600-1040 TF; the uni counted-vmcnt schedule variants measured slower —
# see gemm_uni.hip header); dX and the wide dW go to the gemm_uni TR-mode
# kernels (tr16 transpose-read operands).  hipBLASLt remains only as the
# TFMX_FWD_GEMM=blaslt A/B arm; TFMX_FWD_GEMM=uni forces uni NT forward.
_FWD_BACKEND = os.environ.get("TFMX_FWD_GEMM", "hand")
_FWD_HIP = _FWD_BACKEND == "hip"


# Version counter for weight-derived caches (the padded-transposed logits
# weight): bumped by NoamAdam.step so caches refresh once per step.
_WEIGHT_VERSION = [0]


def bump_weight_version():
    _WEIGHT_VERSION[0] += 1


_WTP_CACHE: dict = {}  # id(weight) -> [version, buf, weight]
_WTP_TABLE = [None]    # cached transpose_batch descriptor table
# A captured hipGraph holds the table ADDRESS it recorded; if the registry
# grows later and the table is rebuilt, the old tensor must stay alive or
# replays would read freed memory.
_WTP_TABLES_KEEP: list = []


def _build_wtp_table(device):
    rows = []
    for ver, buf, w in _WTP_CACHE.values():
        M, N = w.shape
        ldo = buf.stride(0)
        for bm in range(0, M, 64):
            for bn in range(0, N, 64):
                rows.append([w.data_ptr(), buf.data_ptr(), M, N, ldo,
                             bm, bn])
    t = torch.tensor(rows, dtype=torch.int64).to(device)
    _WTP_TABLES_KEEP.append(t)
    return t


def prepare_weight_caches():
    """Build the transpose_batch descriptor table eagerly (it involves a
    host->device copy, which is illegal inside hipGraph capture) — called
    by CapturedTrainStep between warmup and capture."""
    if _WTP_CACHE and _WTP_TABLE[0] is None:
        dev = next(iter(_WTP_CACHE.values()))[1].device
        _WTP_TABLE[0] = _build_wtp_table(dev)


def _wt_padded(E, w, gran=64):
    """W[N,K]^T into a (K, Np) buffer, Np = N rounded up to `gran` (pad
    columns zero) — the NT B-operand for dX.  gran=256 matches ce_bwd's
    padded dlogits contraction (the ragged-vocab head); the generic path
    uses 64 (the GEMM K-step) so the contraction equals dY's width.  All
    registered buffers refresh together in ONE transpose_batch launch per
    optimizer step (bump_weight_version) — a captured step records that
    launch, so graph replays refresh too (graph.py bumps before capture)."""
    key = id(w)
    ent = _WTP_CACHE.get(key)
    npad = (w.shape[0] + gran - 1) // gran * gran
    if ent is None or ent[1].shape[1] != npad:
        buf = torch.zeros(w.shape[1], npad, device=w.device, dtype=w.dtype)
        ent = [_WEIGHT_VERSION[0], buf, w]
        _WTP_CACHE[key] = ent
        _WTP_TABLE[0] = None  # registry changed; rebuild lazily
        E.transpose2d_into(w, buf)
        return buf
    if ent[0] != _WEIGHT_VERSION[0]:
        if _WTP_TABLE[0] is None:
            _WTP_TABLE[0] = _build_wtp_table(w.device)
        E.transpose_batch(_WTP_TABLE[0])
        v = _WEIGHT_VERSION[0]
        for e in _WTP_CACHE.values():
            e[0] = v
    return ent[1]


_CAPTURE_HINT = False


def set_capture_hint(on: bool):
    """Inside a hipGraph (GraphedDecoder) launch overhead is replayed
    away and the library kernels win even at M=B rows (0.705 vs 0.788
    ms/token); eager small-M calls keep the cheap-launch hand-written
    kernel.  Set around warmup+capture so both trace the same path."""
    global _CAPTURE_HINT
    _CAPTURE_HINT = on


def _fwd_gemm(E, x, w, b, activation):
    epi = 1 if activation == "relu" else 0
    if _FWD_BACKEND == "blaslt" and b is not None and \
            (x.shape[0] > 1024 or _CAPTURE_HINT):
        # A/B arm: hipBLASLt fused bias/ReLU epilogues (round-1 default)
        if activation == "relu":
            if hasattr(torch, "_addmm_activation"):
                return torch._addmm_activation(b, x, w.t())
            return torch.relu(torch.nn.functional.linear(x, w, b))
        return torch.nn.functional.linear(x, w, b)
    if _FWD_BACKEND == "uni" and E.gemm_uni_viable(x.shape[0], w.shape[0],
                                                   x.shape[1]):
        return E.gemm_uni_nt(x, w, b, epi)
    # default: gemm256/128 dispatch (best-measured hand-written NT path;
    # launch is cheaper than the library's at small M, decode/serving)
    return E.gemm_nt(x, w, b if b is not None else torch.Tensor(), epi)

def _dw_gemm(dy, x, out=None):
    """dW[N,K] = dY^T @ X — plain GEMM, hand-written both ways: the wide
    logits head goes to the deep-pipelined TRxTR gemm_uni_tn (both
    operands tr16 transpose-read), the d_model-sized heads to the
    split-contraction gemm_dw kernel (tools/gemm_bench.py)."""
    E = ext()
    npad = (dy.shape[1] + 255) // 256 * 256
    if dy.shape[1] >= 8192 and dy.shape[0] % 64 == 0 \
            and (dy.shape[1] % 256 == 0 or dy.stride(0) >= npad) \
            and x.shape[1] % 128 == 0:
        N = dy.shape[1]
        main = (N // 256) * 256
        if main != N and main > 0:
            if out is None:
                out = torch.empty(N, x.shape[1], device=dy.device,
                                  dtype=dy.dtype)
            # Grid-quantization cliff: ceil(N/256) tiles puts the grid a
            # couple of blocks past 256 (one per CU at this kernel's LDS),
            # and the stragglers cost a whole second pass.  Compute the
            # 256-aligned main span at exactly one block wave, then the
            # ragged vocab tail (a few rows, full contraction) split-K so
            # it also fills the chip for its instant of work.
            E.gemm_uni_tn(dy[:, :main], x, out[:main], 1)
            E.gemm_uni_tn(dy[:, main:], x, out[main:], 64)
            return out
        return E.gemm_uni_tn(dy, x, out)
    # gemm_dw writes DISJOINT per-slice fp32 partials (no atomics, no
    # zeroing — the fp32-atomic epilogue measured at the chip's atomic
    # rate); it sizes its own torch::empty workspace via the caching
    # allocator, so no Python-side workspace is needed.
    return E.gemm_dw(dy.contiguous(), x, out, None, None)


# dX backend: "wt" contracts against a per-step cached transposed weight
# through the fast NT path; "uni" reads W red-major via tr16 (no
# transpose); "blaslt" is the library A/B arm.  Default = measured winner.
_DX_BACKEND = os.environ.get("TFMX_DX", "wt")


def _dx_gemm(E, dy, w):
    """dX[M,K] = dY[M,N] @ W[N,K] — hand-written: either NT against the
    cached W^T (refreshed once per optimizer step) or NTxTR with W read
    red-major via tr16.  The ragged-vocab head's dY arrives as ce_bwd's
    zero-padded row-strided view; the contraction widens to the 64-aligned
    pad (zero columns) against the padded-transposed weight."""
    N = w.shape[0]
    M = dy.shape[0]
    if _DX_BACKEND == "blaslt":
        return torch.matmul(dy, w)
    npad = (N + 255) // 256 * 256
    padded = (npad != N and dy.stride(1) == 1 and dy.stride(0) == npad
              and dy.storage_offset() == 0)
    if padded and E.gemm_uni_viable(M, w.shape[1], npad):
        full = dy.as_strided((M, npad), (npad, 1))
        return E.gemm_nt(full, _wt_padded(E, w, 256), torch.Tensor(), 0)
    if _DX_BACKEND == "wt" and N % 64 == 0 and M >= 2048:
        return E.gemm_nt(_dense2d(dy), _wt_padded(E, w), torch.Tensor(), 0)
    if N % 64 == 0 and E.gemm_uni_viable(M, w.shape[1], N):
        return E.gemm_uni_nn(dy, w)
    return torch.matmul(dy, w)  # small/odd shapes (not a training shape)


def _dense2d(t):
    """Row-strided dense (stride(1)==1) passes through — ce_bwd's padded
    dlogits view must NOT be copied back to contiguous."""
    return t if (t.stride(1) == 1 and t.stride(0) >= t.shape[1]) \
        else t.contiguous()


def _dw_db_gemm(dy, x, has_bias, w_out=None, b_out=None):
    """dW and (optionally) db together.  gemm_dw CAN fuse db into its dY
    stream, but the fused variant costs 138 vs 116 VGPRs — one whole
    workgroup of block-level overlap per CU — and measured slower
    end-to-end than a separate colsum pass, so db stays separate."""
    E = ext()
    dw = _dw_gemm(dy, x, out=w_out)
    db = E.colsum(dy, b_out) if has_bias else None
    return dw, db


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, activation):
        # x: (M, K) bf16; w: (N, K) bf16; b: (N,) bf16 or None
        E = ext()
        y = _fwd_gemm(E, x, w, b, activation)
        ctx.activation = activation
        ctx.has_bias = b is not None
        ctx.save_for_backward(x, w, y if activation == "relu" else torch.Tensor())
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        x, w, y = ctx.saved_tensors
        if ctx.activation == "relu":
            # (A fused relu+colsum kernel — relu_bwd_db — was built and
            # measured SLOWER in context at every grid shape: the column-
            # parallel layout + per-column atomics lose to the flat
            # 16k-block stream + separate colsum, the same result as
            # round 1's column-reduction experiments.  docs/PERF.md.)
            dy = E.relu_bwd(dy.contiguous(), y)  # dz = dy * (y > 0)
        else:
            dy = _dense2d(dy)
        dx = _dx_gemm(E, dy, w)         # dX[M,K] = dY[M,N] @ W[N,K]
        dw, db = _dw_db_gemm(dy, x, ctx.has_bias)
        return dx, dw, db, None


class _LinearFlatFn(torch.autograd.Function):
    """Linear whose weight/bias grads go straight into flat-buffer views.

    w/b arrive hidden inside a list so autograd treats only x as
    differentiable; backward writes dW/db into `p._flat_grad` (the kernels'
    `out` argument) and fires the DP readiness callback."""

    @staticmethod
    def forward(ctx, x, wb, activation):
        E = ext()
        w, b = wb
        y = _fwd_gemm(E, x, w, b, activation)
        ctx.activation = activation
        ctx.wb = wb
        ctx.save_for_backward(x, y if activation == "relu" else torch.Tensor())
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        x, y = ctx.saved_tensors
        w, b = ctx.wb
        if ctx.activation == "relu":
            dy = E.relu_bwd(dy.contiguous(), y)
        else:
            dy = _dense2d(dy)
        dx = _dx_gemm(E, dy, w)
        _dw_db_gemm(dy, x, b is not None,
                    w_out=_flat(w).view(w.shape[0], -1),
                    b_out=_flat(b).view(-1) if b is not None else None)
        _grad_ready(w, b)
        return dx, None, None


def linear(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor | None = None,
           activation: str | None = None) -> torch.Tensor:
    """y = x @ W^T + b (+ReLU). x may have leading batch dims."""
    if x.is_cuda:
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        if _flat(w) is not None:
            y = _LinearFlatFn.apply(x2, [w, b], activation)
        else:
            y = _LinearFn.apply(x2, w, b, activation)
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

class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, kv_pad, causal, scale):
        E = ext()
        o, lse = E.attn_fwd(q, k, v,
                            kv_pad if kv_pad is not None else torch.Tensor(),
                            causal, scale)
        ctx.causal = causal
        ctx.scale = scale
        ctx.save_for_backward(q, k, v, o, lse,
                              kv_pad if kv_pad is not None else torch.Tensor())
        return o

    @staticmethod
    def backward(ctx, do):
        E = ext()
        q, k, v, o, lse, kv_pad = ctx.saved_tensors
        dq, dk, dv = E.attn_bwd(q, k, v, o, do.contiguous(), lse, kv_pad,
                                ctx.causal, ctx.scale, 0)
        return dq, dk, dv, None, None, None


class _SelfAttnPackedFn(torch.autograd.Function):
    """Attention straight on the packed (B,S,3,H,dh) QKV tensor: the kernels
    read the q/k/v slots through strides (no contiguous copies) and backward
    writes one packed dQKV (no cat/stack kernels)."""

    @staticmethod
    def forward(ctx, qkv, kv_pad, causal, scale):
        E = ext()
        q, k, v = qkv.unbind(dim=2)  # strided views, never materialized
        o, lse = E.attn_fwd(q, k, v,
                            kv_pad if kv_pad is not None else torch.Tensor(),
                            causal, scale)
        ctx.causal = causal
        ctx.scale = scale
        ctx.save_for_backward(qkv, o, lse,
                              kv_pad if kv_pad is not None else torch.Tensor())
        return o

    @staticmethod
    def backward(ctx, do):
        E = ext()
        qkv, o, lse, kv_pad = ctx.saved_tensors
        q, k, v = qkv.unbind(dim=2)
        (dqkv,) = E.attn_bwd(q, k, v, o, do.contiguous(), lse, kv_pad,
                             ctx.causal, ctx.scale, 1)
        return dqkv, None, None, None


class _CrossAttnPackedFn(torch.autograd.Function):
    """Cross attention: q (B,Sq,H,dh) + packed kv (B,Sk,2,H,dh)."""

    @staticmethod
    def forward(ctx, q, kv, kv_pad, scale):
        E = ext()
        k, v = kv.unbind(dim=2)
        o, lse = E.attn_fwd(q, k, v,
                            kv_pad if kv_pad is not None else torch.Tensor(),
                            False, scale)
        ctx.scale = scale
        ctx.save_for_backward(q, kv, o, lse,
                              kv_pad if kv_pad is not None else torch.Tensor())
        return o

    @staticmethod
    def backward(ctx, do):
        E = ext()
        q, kv, o, lse, kv_pad = ctx.saved_tensors
        k, v = kv.unbind(dim=2)
        dq, dkv = E.attn_bwd(q, k, v, o, do.contiguous(), lse, kv_pad,
                             False, ctx.scale, 2)
        return dq, dkv, None, None


def self_attention(qkv, kv_pad=None, causal=False, return_weights=False):
    """qkv: (B,S,3,H,dh).  GPU path never materializes q/k/v copies."""
    B, S, _, H, dh = qkv.shape
    scale = 1.0 / math.sqrt(dh)
    if qkv.is_cuda and not return_weights:
        kp = kv_pad.to(torch.uint8).contiguous() if kv_pad is not None else None
        return _SelfAttnPackedFn.apply(qkv, kp, causal, scale)
    q, k, v = qkv.unbind(dim=2)
    return fused_attention(q, k, v, kv_pad=kv_pad, causal=causal,
                           return_weights=return_weights)


def cross_attention(q, kv, kv_pad=None, return_weights=False):
    """q: (B,Sq,H,dh); kv: (B,Sk,2,H,dh)."""
    dh = q.shape[-1]
    scale = 1.0 / math.sqrt(dh)
    if q.is_cuda and not return_weights:
        kp = kv_pad.to(torch.uint8).contiguous() if kv_pad is not None else None
        return _CrossAttnPackedFn.apply(q.contiguous(), kv, kp, scale)
    k, v = kv.unbind(dim=2)
    return fused_attention(q, k, v, kv_pad=kv_pad, causal=False,
                           return_weights=return_weights)


def fused_attention(q, k, v, kv_pad=None, causal=False, return_weights=False):
    """q: (B,Sq,H,dh), k/v: (B,Sk,H,dh); kv_pad: (B,Sk) bool/uint8, True=pad.

    Masking semantics match reference Attention.py:25-26: masked logits get
    -1e9 added before softmax. Returns (B,Sq,H,dh); attention weights only on
    the eager/inspection path."""
    scale = 1.0 / math.sqrt(q.shape[-1])
    if q.is_cuda and not return_weights:
        kp = kv_pad.to(torch.uint8).contiguous() if kv_pad is not None else None
        return _AttentionFn.apply(q.contiguous(), k.contiguous(), v.contiguous(),
                                  kp, causal, scale)
    # eager path (CPU, or weight inspection): (B,S,H,dh) -> (B,H,S,dh)
    qt, kt, vt = (t.permute(0, 2, 1, 3) for t in (q, k, v))
    mask = None
    B, Sq, H, _ = q.shape
    Sk = k.shape[1]
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
    out = out.permute(0, 2, 1, 3).to(q.dtype)
    if return_weights:
        return out, w
    return out


# ---------------------------------------------------------------------------
# Fused residual-add + LayerNorm, eps=1e-6 (K9).
# ---------------------------------------------------------------------------

class _ResidualLNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, gamma, beta, eps):
        E = ext()
        y, s, mean, rstd = E.ln_fwd(x, res, gamma, beta, eps)
        ctx.save_for_backward(s, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        s, gamma, mean, rstd = ctx.saved_tensors
        dx, dgamma, dbeta = E.ln_bwd(dy.contiguous(), s, gamma, mean, rstd)
        # d/dx and d/dres are identical (y = LN(x + res))
        return dx, dx, dgamma, dbeta, None


class _ResidualLNFlatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, gb, eps):
        E = ext()
        gamma, beta = gb
        y, s, mean, rstd = E.ln_fwd(x, res, gamma, beta, eps)
        ctx.gb_params = gb
        ctx.save_for_backward(s, gamma, mean, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        s, gamma, mean, rstd = ctx.saved_tensors
        g, b = ctx.gb_params
        dx, _, _ = E.ln_bwd(dy.contiguous(), s, gamma, mean, rstd,
                            _flat(g).view(-1), _flat(b).view(-1))
        _grad_ready(g, b)
        return dx, dx, None, None


class _DropResidualLNFn(torch.autograd.Function):
    """y = LN(dropout(x) + res): the sublayer dropout fused into the LN
    kernels — no standalone dropout read/write of the (B,S,d) tensor in
    either direction."""

    @staticmethod
    def forward(ctx, x, res, gamma, beta, p, eps):
        E = ext()
        if _GRAPH_SEED_T is not None:
            _GRAPH_SALT[0] += 1
            y, s, mean, rstd, mask = E.ln_fwd(x, res, gamma, beta, eps, p,
                                              _GRAPH_SALT[0], _GRAPH_SEED_T)
        else:
            seed = int(torch.randint(0, 2**31 - 1, (1,)).item())
            y, s, mean, rstd, mask = E.ln_fwd(x, res, gamma, beta, eps, p,
                                              seed)
        ctx.p = p
        ctx.flat_gb = None
        ctx.save_for_backward(s, gamma, mean, rstd, mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        s, gamma, mean, rstd, mask = ctx.saved_tensors
        if ctx.flat_gb is not None:
            g, b = ctx.flat_gb
            dres, _, _, dxm = E.ln_bwd(dy.contiguous(), s, gamma, mean, rstd,
                                       _flat(g).view(-1), _flat(b).view(-1),
                                       mask, ctx.p)
            _grad_ready(g, b)
            return dxm, dres, None, None, None, None
        dres, dgamma, dbeta, dxm = E.ln_bwd(dy.contiguous(), s, gamma, mean,
                                            rstd, None, None, mask, ctx.p)
        return dxm, dres, dgamma, dbeta, None, None


class _DropResidualLNFlatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, gb, p, eps):
        y = _DropResidualLNFn.forward(ctx, x, res, gb[0], gb[1], p, eps)
        ctx.flat_gb = gb
        return y

    @staticmethod
    def backward(ctx, dy):
        dxm, dres, _, _, _, _ = _DropResidualLNFn.backward(ctx, dy)
        return dxm, dres, None, None, None


# ---------------------------------------------------------------------------
# Sublayer composites: LN(dropout(linear(x)) + res) and the whole FFN block
# as ONE autograd node each.  Forward runs the same kernels as the separate
# ops (same dropout-seed draws, same order).  Backward starts from the
# one-pass ln_bwd, which already streams dxm — the dY of the linear — and
# so delivers that linear's bias gradient for free (no colsum re-read);
# the FFN block can additionally apply the ReLU mask and the residual-branch
# add in the two dX GEMM epilogues (TFMX_FFN_BWD=fused, default off).
# ---------------------------------------------------------------------------

def _ln_drop_fwd(E, a, res, gamma, beta, eps, p):
    if _GRAPH_SEED_T is not None:
        _GRAPH_SALT[0] += 1
        return E.ln_fwd(a, res, gamma, beta, eps, p, _GRAPH_SALT[0],
                        _GRAPH_SEED_T)
    seed = int(torch.randint(0, 2**31 - 1, (1,)).item())
    return E.ln_fwd(a, res, gamma, beta, eps, p, seed)


def _grad_dst(p, flat):
    """Destination for a 1-D parameter gradient: the flat-buffer view, or
    a fresh tensor handed back to autograd."""
    if p is None:
        return None
    return _flat(p).view(-1) if flat else torch.empty_like(p)


def _ln_drop_bwd(E, ctx, dy, s, gamma, mean, rstd, mask, g, bt, b):
    """Fused ln_bwd writing dgamma/dbeta/db to their destinations.
    Returns (dres, dxm, dgamma, dbeta, db)."""
    flat = ctx.flat
    dg, dbt, db = _grad_dst(g, flat), _grad_dst(bt, flat), _grad_dst(b, flat)
    out = E.ln_bwd(dy.contiguous(), s, gamma, mean, rstd, dg, dbt, mask,
                   ctx.p, db)
    if flat:
        _grad_ready(g, bt)
    return out[0], out[3], dg, dbt, db


class _LinearDropLNFn(torch.autograd.Function):
    """y = LN(dropout(x @ W^T + b) + res)."""

    @staticmethod
    def forward(ctx, x, res, w, b, gamma, beta, p, eps):
        E = ext()
        a = _fwd_gemm(E, x, w, b, None)
        y, s, mean, rstd, mask = _ln_drop_fwd(E, a, res, gamma, beta, eps, p)
        ctx.p = p
        ctx.flat = False
        ctx.params = (w, b, gamma, beta)
        ctx.save_for_backward(x, s, mean, rstd, mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        x, s, mean, rstd, mask = ctx.saved_tensors
        w, b, g, bt = ctx.params
        dres, dxm, dg, dbt, db = _ln_drop_bwd(E, ctx, dy, s, g, mean, rstd,
                                              mask, g, bt, b)
        dx = _dx_gemm(E, dxm, w)
        if ctx.flat:
            _dw_gemm(dxm, x, out=_flat(w).view(w.shape[0], -1))
            _grad_ready(w, b)
            return dx, dres, None, None, None
        dw = _dw_gemm(dxm, x)
        return dx, dres, dw, db, dg, dbt, None, None


class _LinearDropLNFlatFn(torch.autograd.Function):
    """Same, parameters [w, b, gamma, beta] hidden from autograd; their
    gradients land in the flat buffer."""

    @staticmethod
    def forward(ctx, x, res, params, p, eps):
        y = _LinearDropLNFn.forward(ctx, x, res, *params, p, eps)
        ctx.flat = True
        return y

    backward = staticmethod(_LinearDropLNFn.backward)


def _dx_epilogue_ok(E, M, n_out, k):
    """Whether the dX GEMM (M, n_out, k) would run on the gemm256 kernel —
    the only one carrying the relu-mask / residual-add epilogues — through
    the cached-W^T backend.  Opt-in, TFMX_FFN_BWD=fused (A/B arm, read per
    call): with the aux tensor read in the epilogue's 2-byte store pattern
    behind a 1-block/CU main loop, both fused GEMMs measured SLOWER than
    GEMM + separate pass (docs/PERF.md), so the default stays split."""
    return (os.environ.get("TFMX_FFN_BWD", "split") == "fused"
            and _DX_BACKEND == "wt" and M >= 2048
            and n_out % 64 == 0 and k % 64 == 0
            and E.gemm256_viable(M, n_out, k))


class _FFNDropLNFn(torch.autograd.Function):
    """y = LN(dropout(relu(x @ W1^T + b1) @ W2^T + b2) + x)."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2, gamma, beta, p, eps):
        E = ext()
        h = _fwd_gemm(E, x, w1, b1, "relu")
        a = _fwd_gemm(E, h, w2, b2, None)
        y, s, mean, rstd, mask = _ln_drop_fwd(E, a, x, gamma, beta, eps, p)
        ctx.p = p
        ctx.flat = False
        ctx.params = (w1, b1, w2, b2, gamma, beta)
        ctx.save_for_backward(x, h, s, mean, rstd, mask)
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        x, h, s, mean, rstd, mask = ctx.saved_tensors
        w1, b1, w2, b2, g, bt = ctx.params
        flat = ctx.flat
        dres, dxm, dg, dbt, db2 = _ln_drop_bwd(E, ctx, dy, s, g, mean, rstd,
                                               mask, g, bt, b2)
        dw2 = _dw_gemm(dxm, h, out=_flat(w2).view(w2.shape[0], -1)
                       if flat else None)
        if flat:
            _grad_ready(w2, b2)
        M, d, dff = x.shape[0], x.shape[1], h.shape[1]
        nob = torch.Tensor()
        if _dx_epilogue_ok(E, M, dff, d):
            # dz = (dxm @ W2) * (h > 0), mask applied on the accumulators
            dz = E.gemm256_nt(dxm, _wt_padded(E, w2), nob, 2, None, h)
        else:
            dz = E.relu_bwd(_dx_gemm(E, dxm, w2).contiguous(), h)
        dw1 = _dw_gemm(dz, x, out=_flat(w1).view(w1.shape[0], -1)
                       if flat else None)
        db1 = E.colsum(dz, _grad_dst(b1, flat)) if b1 is not None else None
        if flat:
            _grad_ready(w1, b1)
        if _dx_epilogue_ok(E, M, d, dff):
            # dx = dz @ W1 + dres in one rounding
            dx = E.gemm256_nt(dz, _wt_padded(E, w1), nob, 3, None, dres)
        else:
            dx = _dx_gemm(E, dz, w1) + dres
        if flat:
            return dx, None, None, None
        return dx, dw1, db1, dw2, db2, dg, dbt, None, None


class _FFNDropLNFlatFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, params, p, eps):
        y = _FFNDropLNFn.forward(ctx, x, *params, p, eps)
        ctx.flat = True
        return y

    backward = staticmethod(_FFNDropLNFn.backward)


def _all_flat(*params):
    fl = [_flat(p) is not None for p in params if p is not None]
    return all(fl), any(fl)


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
    shp = res.shape
    x2 = x.reshape(-1, x.shape[-1]).contiguous()
    r2 = res.reshape(-1, shp[-1]).contiguous()
    if allf:
        y = _LinearDropLNFlatFn.apply(x2, r2, [w, b, gamma, beta], rate, eps)
    else:
        y = _LinearDropLNFn.apply(x2, r2, w, b, gamma, beta, rate, eps)
    return y.view(shp)


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
    shp = x.shape
    x2 = x.reshape(-1, shp[-1]).contiguous()
    if allf:
        y = _FFNDropLNFlatFn.apply(x2, [w1, b1, w2, b2, gamma, beta], rate,
                                   eps)
    else:
        y = _FFNDropLNFn.apply(x2, w1, b1, w2, b2, gamma, beta, rate, eps)
    return y.view(shp)


def residual_layernorm(x, res, gamma, beta, eps: float = 1e-6):
    if x.is_cuda:
        shp = x.shape
        d = shp[-1]
        x2 = x.reshape(-1, d).contiguous()
        r2 = res.reshape(-1, d).contiguous()
        if _flat(gamma) is not None:
            y = _ResidualLNFlatFn.apply(x2, r2, [gamma, beta], eps)
        else:
            y = _ResidualLNFn.apply(x2, r2, gamma, beta, eps)
        return y.view(shp)
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
        shp = x.shape
        d = shp[-1]
        x2 = x.reshape(-1, d).contiguous()
        r2 = res.reshape(-1, d).contiguous()
        if _flat(gamma) is not None:
            y = _DropResidualLNFlatFn.apply(x2, r2, [gamma, beta], rate, eps)
        else:
            y = _DropResidualLNFn.apply(x2, r2, gamma, beta, rate, eps)
        return y.view(shp)
    xd = torch.nn.functional.dropout(x, p=rate, training=True)
    return residual_layernorm(xd, res, gamma, beta, eps)


# ---------------------------------------------------------------------------
# Fused embedding * sqrt(d) + positional encoding (K10).
# ---------------------------------------------------------------------------

class _EmbedPEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, tokens, weight, pe):
        E = ext()
        y = E.embed_pe_fwd(tokens, weight, pe)
        ctx.vocab = weight.shape[0]
        ctx.save_for_backward(tokens)
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        (tokens,) = ctx.saved_tensors
        dw = E.embed_pe_bwd(dy.contiguous(), tokens, ctx.vocab)
        return None, dw, None


class _EmbedPEFlatFn(torch.autograd.Function):
    """Embedding fwd with dW scatter-add cast straight into the flat view.
    Output still requires grad (x flows onward), so a dummy differentiable
    input threads the graph."""

    @staticmethod
    def forward(ctx, marker, tokens, wref, pe):
        E = ext()
        (weight,) = wref
        y = E.embed_pe_fwd(tokens, weight, pe)
        ctx.vocab = weight.shape[0]
        ctx.wref = wref
        ctx.save_for_backward(tokens)
        return y

    @staticmethod
    def backward(ctx, dy):
        E = ext()
        (tokens,) = ctx.saved_tensors
        (weight,) = ctx.wref
        E.embed_pe_bwd(dy.contiguous(), tokens, ctx.vocab,
                       _flat(weight).view(-1))
        _grad_ready(weight)
        return None, None, None, None


def embedding_scale_pe_at(tokens, weight, pe, pos: int):
    """Embedding + PE for an incremental decode step: positions start at
    `pos` instead of 0 (KV-cache path)."""
    return embedding_scale_pe(tokens, weight,
                              pe[pos:pos + tokens.shape[1]].contiguous())


def embedding_scale_pe(tokens, weight, pe):
    """tokens (B,S) int; weight (V,d); pe (P,d) fp32 table, P >= S."""
    if weight.is_cuda:
        if _flat(weight) is not None and torch.is_grad_enabled():
            marker = torch.empty(0, device=weight.device,
                                 dtype=weight.dtype, requires_grad=True)
            return _EmbedPEFlatFn.apply(marker, tokens.contiguous(),
                                        [weight], pe)
        return _EmbedPEFn.apply(tokens.contiguous(), weight, pe)
    if weight.dtype in (torch.bfloat16, torch.float16):
        return R.embedding_scale_pe(tokens, weight.float(), pe[None].float()).to(weight.dtype)
    return R.embedding_scale_pe(tokens, weight, pe[None].to(weight.dtype))


# ---------------------------------------------------------------------------
# Dropout (K11): mask saved for exact backward; seeds from torch RNG.
# ---------------------------------------------------------------------------

# HIP-graph capture support: while a step is being
# captured, dropout seeds must come from a DEVICE counter (advanced
# in-graph by the optimizer's adam_coefs kernel) — a host seed would be
# baked into the graph and every replay would reuse the same mask.  Each
# call site gets a distinct salt (capture-order is deterministic).
_GRAPH_SEED_T = None
_GRAPH_SALT = [0]


def set_graph_rng(seed_tensor):
    """Install (or clear, with None) the device seed tensor used by dropout
    during graph capture."""
    global _GRAPH_SEED_T
    _GRAPH_SEED_T = seed_tensor
    _GRAPH_SALT[0] = 0


class _DropoutFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p):
        E = ext()
        if _GRAPH_SEED_T is not None:
            _GRAPH_SALT[0] += 1
            y, mask = E.dropout_fwd(x, p, _GRAPH_SALT[0], _GRAPH_SEED_T)
        else:
            seed = int(torch.randint(0, 2**31 - 1, (1,)).item())
            y, mask = E.dropout_fwd(x, p, seed)
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
        B = logits.shape
        V = logits.shape[-1]
        correct, total = ext().accuracy(logits.reshape(-1, V).contiguous(),
                                        targets.reshape(-1).contiguous())
        return float(correct), float(total)
    pred = logits.argmax(dim=-1)
    mask = targets != 0
    return (float(((pred == targets) & mask).sum()), float(mask.sum()))
