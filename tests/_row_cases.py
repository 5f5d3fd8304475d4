"""Inputs, fp64 references and bound checks of the row-kernel tests.

Shared by tests/test_gpu_row_kernels.py (the HIP kernels) and
tests/test_row_kernel_bounds.py (a plain fp32 torch emulation on the CPU):
both build the same bf16 inputs from a CPU torch.Generator and hand their
outputs, as CPU tensors, to the same check_* functions.  Every reference is
fp64 on the bf16 values the kernel received.

Bound form (tests/_gpu_bounds.py): |got - ref| <= u*|ref| + 1e-5*absterm,
u = 2^-8 the bf16 unit roundoff, absterm the sum of magnitudes of the terms
the kernel adds; fp32 outputs drop the u term."""

import functools
import math

import torch

from _gpu_bounds import (U, _check_f32, _check_lim, _check_u,
                         dropout_inv_keep, dropout_keep)

LN_EPS = 1e-6


def _bits(t):
    return t.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------

CE_BATCH = 8.0
CE_VOCABS = [5, 1003, 2048, 2056, 4099, 32770]
CE_SHAPES = [(9, v) for v in CE_VOCABS] + [(300, 16)]


@functools.lru_cache(maxsize=None)
def ce_case(R, V, seed=0):
    """Rows 0-8: 0 pad target; 1 zeros with one +30 at V//2 (softmax ~1 at a
    non-target); 2 shifted by +100; 3 constant; 4 maximum in the last
    column; 5 target V-1; 6/7 targets 7 and 8 (the two sides of the first
    8-vector boundary); the rest randn*2 with targets in [1, V), and past
    row 8 every fifth target a pad."""
    assert R >= 9 and V >= 5
    g = torch.Generator().manual_seed(1000 * seed + V)
    x = torch.randn(R, V, generator=g) * 2
    tgt = torch.randint(1, V, (R,), generator=g)
    x[1] = 0.0
    x[1, V // 2] = 30.0
    x[2] += 100.0
    x[3] = 0.75
    x[4, V - 1] = x[4].max() + 3.0
    tgt[0] = 0
    tgt[1] = 1                      # V // 2 >= 2
    tgt[5] = V - 1
    if V >= 9:
        tgt[6], tgt[7] = 7, 8
    tgt[9::5] = 0
    return dict(x=x.bfloat16(), tgt=tgt, R=R, V=V)


@functools.lru_cache(maxsize=None)
def ce_ref(R, V, eps, seed=0):
    c = ce_case(R, V, seed)
    x = c["x"].double()
    tgt = c["tgt"]
    lse = torch.logsumexp(x, -1)
    mask = (tgt != 0).double()
    xt = x.gather(1, tgt[:, None])[:, 0]
    per_row = (1 - eps) * (lse - xt) + eps * (lse - x.mean(-1))
    loss = (mask * per_row).sum() / CE_BATCH
    loss_abs = (mask * (lse.abs() + xt.abs() + eps * x.abs().mean(-1))).sum() \
        / CE_BATCH
    onehot = torch.zeros_like(x)
    onehot[torch.arange(R), tgt] = 1.0
    sm = torch.exp(x - lse[:, None])
    # unit-seed gradient and its absterm; (1 + |lse|): the stored fp32 lse
    # carries a representation error that is a relative error of the softmax
    grad = mask[:, None] * (sm - eps / V - (1 - eps) * onehot) / CE_BATCH
    grad_abs = mask[:, None] * (sm * (1 + lse.abs()[:, None]) + eps / V
                                + (1 - eps) * onehot) / CE_BATCH
    return dict(lse=lse, loss=loss, loss_abs=loss_abs, grad=grad,
                grad_abs=grad_abs)


def check_ce_fwd(R, V, eps, lse, loss, tag, seed=0):
    r = ce_ref(R, V, eps, seed)
    if lse is not None:
        assert lse.dtype == torch.float32
        _check_f32(lse, r["lse"], 1 + r["lse"].abs(), f"{tag} lse")
    assert loss.dtype == torch.float32
    _check_f32(loss.reshape(()), r["loss"], r["loss_abs"], f"{tag} loss")


def check_ce_grad(R, V, eps, full, dloss, tag, u=U, seed=0):
    """full: the (R, roundup(V, 256)) tensor the kernels return."""
    c, r = ce_case(R, V, seed), ce_ref(R, V, eps, seed)
    Vp = (V + 255) // 256 * 256
    assert full.dtype == torch.bfloat16
    assert tuple(full.shape) == (R, Vp), (tag, tuple(full.shape))
    assert bool((_bits(full[:, V:]) == 0).all()), f"{tag}: pad columns"
    assert bool((_bits(full[c["tgt"] == 0]) == 0).all()), f"{tag}: pad rows"
    _check_u(full[:, :V], r["grad"] * dloss, r["grad_abs"] * abs(dloss),
             f"{tag} grad", u=u)


def ce_emulate(R, V, eps, dloss=1.0, perturb=None, seed=0):
    """The kernels' arithmetic in plain fp32 torch: (loss, lse, full)."""
    c = ce_case(R, V, seed)
    x, tgt = c["x"].float(), c["tgt"]
    f32 = torch.float32
    eps_t = torch.tensor(eps, dtype=f32)
    batch = CE_BATCH + 1 if perturb == "batch_plus_1" else CE_BATCH
    inv_batch = torch.tensor(1.0, dtype=f32) / torch.tensor(batch, dtype=f32)
    lse = torch.logsumexp(x, -1)
    mask = tgt != 0
    xt = x.gather(1, tgt[:, None])[:, 0]
    per_row = lse - (1 - eps_t) * xt - eps_t * (x.sum(-1) / V)
    loss = torch.where(mask, per_row * inv_batch, torch.zeros(())).sum()
    onehot = torch.zeros_like(x)
    onehot[torch.arange(R), tgt] = 1.0
    eps_v = torch.zeros((), dtype=f32) if perturb == "no_eps_v" else eps_t / V
    g = torch.exp(x - lse[:, None]) - eps_v - onehot * (1 - eps_t)
    g = g * (torch.tensor(dloss, dtype=f32) * inv_batch)
    g = torch.where(mask[:, None], g, torch.zeros(()))
    assert loss.dtype == f32 and g.dtype == f32
    full = torch.zeros(R, (V + 255) // 256 * 256, dtype=torch.bfloat16)
    full[:, :V] = g.bfloat16()
    return loss, lse, full


# ---------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------

LN_SHAPES = [(5, 8), (7, 100), (6, 101), (9, 520), (5, 1024), (5, 1032),
             (130, 96)]
LN_DROP_SHAPES = [(7, 100), (9, 520), (5, 1032)]
LN_P = 0.3
LN_SEED = 1234


@functools.lru_cache(maxsize=None)
def ln_case(R, D):
    """R rows of x ~ N(0 or 8 alternating, 1) and one more, the last, with
    x = 1.5 and res = 0.5: constant and exactly representable."""
    g = torch.Generator().manual_seed(100000 + 1000 * R + D)

    def rn(*s):
        return torch.randn(*s, generator=g)
    x = rn(R + 1, D)
    x[1::2] += 8.0
    res = rn(R + 1, D)
    x[R], res[R] = 1.5, 0.5
    return dict(x=x.bfloat16(), res=res.bfloat16(), gamma=rn(D).bfloat16(),
                beta=rn(D).bfloat16(), dy=rn(R + 1, D).bfloat16(), R=R, D=D)


def ln_mask(R, D, counter=None):
    """Oracle keep mask of the fused dropout, (R+1, D) uint8."""
    m = dropout_keep((R + 1) * D, LN_P, LN_SEED, counter)
    return torch.from_numpy(m).view(R + 1, D)


def check_ln_fwd(R, D, y, s, mean, rstd, tag, mask=None):
    """mask None: no dropout.  Else the (R+1)*D byte mask the kernel wrote;
    it must equal the oracle, and s, mean, rstd, y follow from it."""
    c = ln_case(R, D)
    x, res = c["x"].double(), c["res"].double()
    gamma, beta = c["gamma"].double(), c["beta"].double()
    assert mean.dtype == torch.float32 and rstd.dtype == torch.float32
    rows = slice(0, R + 1)
    if mask is None:
        t = x + res
        assert torch.equal(_bits(s),
                           _bits((c["x"].float() + c["res"].float())
                                 .bfloat16())), f"{tag}: s"
        rows = slice(0, R)      # rstd of the constant row: var is 0
    else:
        mk = ln_mask(R, D)
        assert mask.dtype == torch.uint8
        assert torch.equal(mask.view(R + 1, D), mk), f"{tag}: mask"
        xk = mk.double() * x * dropout_inv_keep(LN_P)
        t = xk + res
        _check_u(s, t, xk.abs() + res.abs(), f"{tag} s")
    m = t.mean(-1)
    var = ((t - m[:, None]) ** 2).mean(-1)
    rs = 1.0 / torch.sqrt(var + LN_EPS)
    xhat = (t - m[:, None]) * rs[:, None]
    _check_f32(mean, m, t.abs().mean(-1), f"{tag} mean")
    # conditioning of the one-pass variance E[t^2] - mean^2 (each term's
    # fp32 error is relative to the term, var is their difference) plus the
    # hardware rsqrt
    cond = ((t * t).mean(-1) + m * m) / (var + LN_EPS)
    _check_lim((rstd.double() / rs)[rows], torch.ones_like(rs)[rows],
               (1e-5 * cond + 2.0 ** -22)[rows], f"{tag} rstd")
    # y normalises the bf16-rounded s with the statistics of the un-rounded
    # t: the rounding of s, <= u*|t|, is scaled by rstd*|gamma|
    _check_u(y, xhat * gamma + beta, (xhat * gamma).abs() + beta.abs(),
             f"{tag} y", extra=U * t.abs() * rs[:, None] * gamma.abs())
    if mask is None:
        assert torch.equal(_bits(y[R]), _bits(c["beta"])), \
            f"{tag}: y of the constant row is not beta"


def check_ln_bwd(R, D, s, mean, rstd, out, tag, mask=None):
    """out = ln_bwd's list.  The reference is built from the saved s and the
    kernel's own mean / rstd, which isolates the backward."""
    c = ln_case(R, D)
    dy, gamma = c["dy"].double(), c["gamma"].double()
    mu, rs = mean.double()[:, None], rstd.double()[:, None]
    xh = (s.double() - mu) * rs
    g = dy * gamma
    dx = rs * (g - g.mean(-1, keepdim=True)
               - xh * (g * xh).mean(-1, keepdim=True))
    dx_abs = rs * (g.abs() + g.abs().mean(-1, keepdim=True)
                   + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
    for o in out:
        assert o.dtype == torch.bfloat16
        assert bool(torch.isfinite(o.float()).all()), f"{tag}: non-finite"
    _check_u(out[0], dx, dx_abs, f"{tag} dx")
    tg = dy * xh
    _check_u(out[1], tg.sum(0), tg.abs().sum(0), f"{tag} dgamma")
    _check_u(out[2], dy.sum(0), dy.abs().sum(0), f"{tag} dbeta")
    if mask is not None:
        ik = dropout_inv_keep(LN_P)
        keep = mask.view(R + 1, D) != 0
        dxm = out[3]
        assert bool((_bits(dxm)[~keep] == 0).all()), f"{tag}: dxm at drops"
        _check_u(torch.where(keep, dxm.double(), 0.0),
                 torch.where(keep, dx * ik, 0.0), dx_abs * ik, f"{tag} dxm")
        if len(out) > 4:
            d = dxm.double()
            _check_u(out[4], d.sum(0), d.abs().sum(0), f"{tag} dbias")


def ln_emulate_fwd(R, D, drop=False, perturb=None):
    """ln_fwd in plain fp32 torch, in the kernel's order of operations:
    (y, s, mean, rstd[, mask])."""
    c = ln_case(R, D)
    x, res = c["x"].float(), c["res"].float()
    mk = None
    if drop:
        mk = ln_mask(R, D)
        x = torch.where(mk != 0, x * dropout_inv_keep(LN_P), torch.zeros(()))
    t = x + res
    s = t.bfloat16()
    mean = t.sum(-1) / D
    var = ((t * t).sum(-1) / D - mean * mean).clamp(min=0.0)
    if perturb == "var_d_minus_1":
        var = var * D / (D - 1)
    rstd = torch.rsqrt(var + LN_EPS)
    y = ((s.float() - mean[:, None]) * rstd[:, None] * c["gamma"].float()
         + c["beta"].float()).bfloat16()
    assert t.dtype == torch.float32 and rstd.dtype == torch.float32
    return (y, s, mean, rstd) + ((mk.reshape(-1),) if drop else ())


def ln_emulate_bwd(R, D, s, mean, rstd, mask=None):
    c = ln_case(R, D)
    dy, gamma = c["dy"].float(), c["gamma"].float()
    mu, rs = mean[:, None], rstd[:, None]
    xh = (s.float() - mu) * rs
    g = dy * gamma
    d = rs * (g - g.sum(-1, keepdim=True) / D
              - xh * ((g * xh).sum(-1, keepdim=True) / D))
    assert d.dtype == torch.float32
    out = [d.bfloat16(), (dy * xh).sum(0).bfloat16(), dy.sum(0).bfloat16()]
    if mask is not None:
        keep = mask.view(R + 1, D) != 0
        dxm = torch.where(keep, d * dropout_inv_keep(LN_P),
                          torch.zeros(())).bfloat16()
        out += [dxm, dxm.float().sum(0).bfloat16()]
    return out


# ---------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------

DROP_NS = [1, 3, 4, 5, 1023, 1024, 1027]
DROP_SEED = 4321


@functools.lru_cache(maxsize=None)
def dropout_case(n):
    g = torch.Generator().manual_seed(7000 + n)
    return dict(x=torch.randn(n, generator=g).bfloat16(),
                dy=torch.randn(n, generator=g).bfloat16())


def dropout_expected(v, mask, p):
    """where(mask, bf16(v * inv_keep), +0), v bf16."""
    scaled = (v.float() * dropout_inv_keep(p)).bfloat16()
    return torch.where(mask != 0, scaled, torch.zeros((), dtype=scaled.dtype))


def check_dropout(n, p, y, mask, dx, tag, counter=None):
    c = dropout_case(n)
    want = torch.from_numpy(dropout_keep(n, p, DROP_SEED, counter))
    assert mask.dtype == torch.uint8 and mask.shape == (n,)
    assert torch.equal(mask, want), f"{tag}: mask differs from the oracle"
    assert torch.equal(_bits(y), _bits(dropout_expected(c["x"], want, p))), \
        f"{tag}: y"
    if dx is not None:
        assert torch.equal(_bits(dx),
                           _bits(dropout_expected(c["dy"], want, p))), \
            f"{tag}: dx"


# ---------------------------------------------------------------------------
# embedding
# ---------------------------------------------------------------------------

EMB_V = 50
EMB_PE_ROWS = 12
EMB_TOKENS = [0, EMB_V - 1, 3, 3, 17, EMB_V - 1, 0]
EMB_POSITIONS = [0, 11, 5, 5, 2, 0, 1]
EMB_BWD_PATTERNS = ["same", "three", "distinct"]


@functools.lru_cache(maxsize=None)
def emb_case(D):
    g = torch.Generator().manual_seed(300 + D)
    return dict(w=torch.randn(EMB_V, D, generator=g).bfloat16(),
                pe=torch.randn(EMB_PE_ROWS, D, generator=g).bfloat16(),
                tokens=torch.tensor([EMB_TOKENS]),
                positions=torch.tensor([EMB_POSITIONS], dtype=torch.int32))


def check_emb_fwd(D, y, tag, positions):
    c = emb_case(D)
    S = len(EMB_TOKENS)
    assert tuple(y.shape) == (1, S, D) and y.dtype == torch.bfloat16
    pos = c["positions"][0].long() if positions else torch.arange(S)
    w = c["w"].double()[c["tokens"][0]]
    pe = c["pe"].double()[pos]
    sq = math.sqrt(D)
    _check_u(y[0], w * sq + pe, w.abs() * sq + pe.abs(), f"{tag} y")


def emb_emulate_fwd(D, positions):
    c = emb_case(D)
    S = len(EMB_TOKENS)
    pos = c["positions"][0].long() if positions else torch.arange(S)
    scale = torch.tensor(float(D), dtype=torch.float32).sqrt()
    y = c["w"].float()[c["tokens"][0]] * scale + c["pe"].float()[pos]
    return y.bfloat16()[None]


@functools.lru_cache(maxsize=None)
def emb_bwd_case(D, pattern):
    g = torch.Generator().manual_seed(900 + D)
    if pattern == "same":           # maximal atomic contention
        tokens = torch.full((300,), 5)
    elif pattern == "three":
        tokens = torch.tensor([0, 7, EMB_V - 1])[
            torch.randint(0, 3, (300,), generator=g)]
    else:
        tokens = torch.tensor([4, 0, 49, 13, 2, 31, 8])
    n = tokens.numel()
    return dict(tokens=tokens.view(1, n),
                dy=torch.randn(1, n, D, generator=g).bfloat16())


def check_emb_bwd(D, pattern, dw, tag):
    c = emb_bwd_case(D, pattern)
    tok, dy = c["tokens"][0], c["dy"][0].double()
    assert tuple(dw.shape) == (EMB_V, D) and dw.dtype == torch.bfloat16
    sq = math.sqrt(D)
    ref = torch.zeros(EMB_V, D, dtype=torch.float64).index_add_(0, tok, dy * sq)
    ab = torch.zeros(EMB_V, D, dtype=torch.float64) \
        .index_add_(0, tok, dy.abs() * sq)
    _check_u(dw, ref, ab, f"{tag} dw")
    unused = torch.ones(EMB_V, dtype=torch.bool)
    unused[tok] = False
    assert bool((_bits(dw)[unused] == 0).all()), f"{tag}: unused token rows"


def emb_emulate_bwd(D, pattern):
    c = emb_bwd_case(D, pattern)
    scale = torch.tensor(float(D), dtype=torch.float32).sqrt()
    return torch.zeros(EMB_V, D).index_add_(
        0, c["tokens"][0], c["dy"][0].float() * scale).bfloat16()


# ---------------------------------------------------------------------------
# argmax / accuracy
# ---------------------------------------------------------------------------

ARGMAX_VS = [1, 63, 64, 65, 1003]


def lowest_argmax(x):
    """Lowest index among the row maxima, written out (not torch.argmax)."""
    V = x.shape[-1]
    x = x.float()
    idx = torch.arange(V).expand_as(x)
    hit = x == x.max(-1, keepdim=True).values
    return torch.where(hit, idx, torch.full_like(idx, V)).min(-1).values


def highest_argmax(x):
    x = x.float()
    idx = torch.arange(x.shape[-1]).expand_as(x)
    hit = x == x.max(-1, keepdim=True).values
    return torch.where(hit, idx, torch.full_like(idx, -1)).max(-1).values


@functools.lru_cache(maxsize=None)
def argmax_case(V):
    """bf16 logits and (hit, miss) target vectors.  Rows: all equal; the
    maximum twice, at (5, V-1), at (63, 64) (neighbouring lanes) and at
    (64, 127) (lane 0 twice, then lane 63), where the columns exist; the
    maximum at V-1; all negative; a randn block."""
    g = torch.Generator().manual_seed(40 + V)
    rows, ties = [], []

    def base():
        return torch.randn(V, generator=g)

    def add(row, tie=None):         # tie: the higher index of a made tie
        rows.append(row)
        ties.append(tie)
    add(torch.full((V,), 0.5), V - 1)
    for a, b in [(5, V - 1), (63, 64), (64, 127)]:
        if a < b < V:
            r = base()
            r[a] = r[b] = 9.0
            add(r, b)
    r = base()
    r[V - 1] = 9.0
    add(r)
    for _ in range(2):
        add(-base().abs() - 1.0)
    r = -base().abs() - 1.0
    if V > 40:
        r[3] = r[40] = -0.5         # an all-negative tie
    add(r, 40 if V > 40 else None)
    for _ in range(8):
        add(base())
    x = torch.stack(rows).bfloat16()
    ref = lowest_argmax(x)
    # miss: the other tied index where there is one, else a neighbour
    miss = torch.tensor([t if t is not None else (int(i) + 1) % V
                         for t, i in zip(ties, ref)])
    made = torch.tensor([t is not None for t in ties])
    return dict(x=x, ref=ref, hit=ref.clone(), miss=miss, made_tie=made)


def accuracy_ref(x, targets):
    mask = targets != 0
    return (int(((lowest_argmax(x) == targets) & mask).sum()),
            int(mask.sum()))
