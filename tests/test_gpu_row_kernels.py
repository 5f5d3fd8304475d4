"""Row kernels against fp64 references, element-wise: layernorm.hip
(ln_fwd / ln_bwd), cross_entropy.hip (ce_fwd / ce_bwd / ce_fused /
ce_scale), embedding.hip, dropout.hip and reduce.hip (argmax_lastdim /
accuracy).

Inputs, references and bounds live in tests/_row_cases.py and are shared
with tests/test_row_kernel_bounds.py, which shows on the CPU that each bound
admits a plain fp32 evaluation and rejects a subtly wrong one.  The bounds
were derived from the fp32 unit roundoff and the depth of the sums, not
fitted to what the kernels produce; every check prints its worst err/limit.

Worst err/limit measured on an MI355X over all cases (1 is the bound; the
bf16 outputs sit where the CPU emulation does, at the rounding itself):
    ce   lse 0.0101  loss 0.0032  grad (ce_bwd, ce_fused) 0.9919
         ce_fused vs ce_bwd 0.0000  ce_fused+ce_scale (2u) 0.8674
    ln   mean 0.0101  rstd 0.0089  y 0.9952  s (dropout) 0.9816
         dx 0.9882  dgamma 0.9854  dbeta 0.9927  dxm 0.9811  dbias 0.9805
    embedding  y 0.9918  dw 0.9636
"""

import pytest
import torch

import _row_cases as C
from _gpu_bounds import U, _check_pair, _env

pytestmark = pytest.mark.gpu


def _ext():
    from transformer_amd.ops import ext
    return ext()


def _dev(*ts):
    return [t.cuda() for t in ts]


def _scalar(v):
    return torch.full((1,), v, device="cuda", dtype=torch.float32)


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("R,V", C.CE_SHAPES)
def test_ce(R, V, eps):
    E = _ext()
    c = C.ce_case(R, V)
    x, tgt = _dev(c["x"], c["tgt"])
    tag = f"ce R={R} V={V} eps={eps}"

    loss, lse = E.ce_fwd(x, tgt, C.CE_BATCH, eps)
    C.check_ce_fwd(R, V, eps, lse.cpu(), loss.cpu(), tag + " ce_fwd")
    g1 = E.ce_bwd(x, tgt, lse, _scalar(1.0), C.CE_BATCH, eps)
    C.check_ce_grad(R, V, eps, g1.cpu(), 1.0, tag + " ce_bwd")
    g25 = E.ce_bwd(x, tgt, lse, _scalar(2.5), C.CE_BATCH, eps)
    C.check_ce_grad(R, V, eps, g25.cpu(), 2.5, tag + " ce_bwd dloss=2.5")

    lossf, gf = E.ce_fused(x, tgt, C.CE_BATCH, eps)
    C.check_ce_fwd(R, V, eps, None, lossf.cpu(), tag + " ce_fused")
    C.check_ce_grad(R, V, eps, gf.cpu(), 1.0, tag + " ce_fused")
    _check_pair(gf[:, :V], g1[:, :V], tag + " ce_fused vs ce_bwd")
    # a unit seed leaves the gradient alone; 2.5 rounds to bf16 a second time
    keep = gf.clone()
    E.ce_scale(gf, _scalar(1.0))
    assert torch.equal(gf.view(torch.int16), keep.view(torch.int16))
    E.ce_scale(gf, _scalar(2.5))
    C.check_ce_grad(R, V, eps, gf.cpu(), 2.5, tag + " ce_fused+ce_scale",
                    u=2 * U)


@pytest.mark.parametrize("fused", [False, True])
def test_ce_loss_banks_rezeroed(fused):
    """Two calls in a row on different data through the cached 256 loss
    banks (300 rows wrap them): the second loss meets its own bound only if
    the first call left the banks zero."""
    E = _ext()
    R, V, eps = 300, 16, 0.1
    losses = []
    for seed in (0, 1):
        c = C.ce_case(R, V, seed)
        x, tgt = _dev(c["x"], c["tgt"])
        fn = E.ce_fused if fused else E.ce_fwd
        losses.append(fn(x, tgt, C.CE_BATCH, eps)[0])
    for seed, loss in enumerate(losses):
        C.check_ce_fwd(R, V, eps, None, loss.cpu(),
                       f"banks fused={fused} call {seed}", seed=seed)


# ---------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------

_LN_ARMS = {"default": {}, "split": {"TFMX_LN_BWD": "split"},
            "waves8": {"TFMX_LN_BWD_WAVES": "8"}}


def _ln_inputs(R, D):
    c = C.ln_case(R, D)
    return _dev(c["x"], c["res"], c["gamma"], c["beta"], c["dy"])


def _cpu(ts):
    return [t.cpu() for t in ts]


# the 8-wave variant is a choice only where D <= 512
@pytest.mark.parametrize("R,D,arm", [
    (R, D, arm) for R, D in C.LN_SHAPES for arm in _LN_ARMS
    if arm != "waves8" or D <= 512])
def test_ln(R, D, arm):
    """D % 8 != 0 takes the scalar paths of ln_fwd / ln_bwd, where each lane
    once ran past its own 8 columns to the end of the row: mean came out
    several times too large (err/limit 6e5 at D = 100) with nothing else in
    the suite looking at it."""
    E = _ext()
    x, res, gamma, beta, dy = _ln_inputs(R, D)
    tag = f"ln R={R} D={D} {arm}"
    y, s, mean, rstd = E.ln_fwd(x, res, gamma, beta, C.LN_EPS, 0.0, 0, None)
    C.check_ln_fwd(R, D, *_cpu([y, s, mean, rstd]), tag)
    with _env(TFMX_LN_BWD=None, TFMX_LN_BWD_WAVES=None):
        with _env(**_LN_ARMS[arm]):
            out = E.ln_bwd(dy, s, gamma, mean, rstd)
    assert len(out) == 3
    C.check_ln_bwd(R, D, *_cpu([s, mean, rstd]), _cpu(out), tag)


@pytest.mark.parametrize("arm", ["default", "split"])
@pytest.mark.parametrize("R,D", C.LN_DROP_SHAPES)
def test_ln_dropout(R, D, arm):
    E = _ext()
    x, res, gamma, beta, dy = _ln_inputs(R, D)
    tag = f"ln drop R={R} D={D} {arm}"
    y, s, mean, rstd, mask = E.ln_fwd(x, res, gamma, beta, C.LN_EPS, C.LN_P,
                                      C.LN_SEED, None)
    C.check_ln_fwd(R, D, *_cpu([y, s, mean, rstd]), tag, mask=mask.cpu())
    db = torch.empty(D, device="cuda", dtype=torch.bfloat16)
    with _env(TFMX_LN_BWD=None, TFMX_LN_BWD_WAVES=None):
        with _env(**_LN_ARMS[arm]):
            out5 = E.ln_bwd(dy, s, gamma, mean, rstd, None, None, mask,
                            C.LN_P, db)
            out4 = E.ln_bwd(dy, s, gamma, mean, rstd, None, None, mask,
                            C.LN_P)
    assert len(out5) == 5 and out5[4].data_ptr() == db.data_ptr()
    assert len(out4) == 4
    sc, mc, rc, kc = _cpu([s, mean, rstd, mask])
    C.check_ln_bwd(R, D, sc, mc, rc, _cpu(out5), tag + " +dbias", mask=kc)
    C.check_ln_bwd(R, D, sc, mc, rc, _cpu(out4), tag, mask=kc)


def test_ln_dropout_device_counter():
    """seed_t: the mask follows the device counter, by the oracle's rule."""
    E = _ext()
    R, D = 7, 100
    x, res, gamma, beta, _ = _ln_inputs(R, D)
    masks = []
    for k in (3, 4):
        st = torch.tensor([k], device="cuda", dtype=torch.int64)
        out = E.ln_fwd(x, res, gamma, beta, C.LN_EPS, C.LN_P, C.LN_SEED, st)
        masks.append(out[4].cpu().view(R + 1, D))
        assert torch.equal(masks[-1], C.ln_mask(R, D, counter=k)), k
    assert not torch.equal(masks[0], masks[1])


# ---------------------------------------------------------------------------
# dropout
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("n", C.DROP_NS)
def test_dropout(n, p):
    E = _ext()
    c = C.dropout_case(n)
    x, dy = _dev(c["x"], c["dy"])
    y, mask = E.dropout_fwd(x, p, C.DROP_SEED)
    dx = E.dropout_bwd(dy, mask, p)
    C.check_dropout(n, p, y.cpu(), mask.cpu(), dx.cpu(), f"dropout n={n} p={p}")


@pytest.mark.parametrize("n", [5, 1027])
def test_dropout_rate_zero(n):
    x, = _dev(C.dropout_case(n)["x"])
    y, mask = _ext().dropout_fwd(x, 0.0, C.DROP_SEED)
    assert bool((mask == 1).all())
    assert torch.equal(y.view(torch.int16), x.view(torch.int16))


def test_dropout_device_counter():
    E = _ext()
    n, p = 1027, 0.5
    x, = _dev(C.dropout_case(n)["x"])
    masks = []
    for k in (3, 4):
        st = torch.tensor([k], device="cuda", dtype=torch.int64)
        y, mask = E.dropout_fwd(x, p, C.DROP_SEED, seed_t=st)
        C.check_dropout(n, p, y.cpu(), mask.cpu(), None, f"seed_t={k}",
                        counter=k)
        masks.append(mask.cpu())
    assert not torch.equal(masks[0], masks[1])


# ---------------------------------------------------------------------------
# embedding
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("positions", [False, True])
@pytest.mark.parametrize("D", [8, 100, 512, 520])
def test_embedding_fwd(D, positions):
    c = C.emb_case(D)
    assert c["pe"].shape[0] > c["tokens"].shape[1]
    tokens, w, pe, pos = _dev(c["tokens"], c["w"], c["pe"], c["positions"])
    y = _ext().embed_pe_fwd(tokens, w, pe, pos if positions else None)
    C.check_emb_fwd(D, y.cpu(), f"embed D={D} positions={positions}",
                    positions)


@pytest.mark.parametrize("pattern", C.EMB_BWD_PATTERNS)
@pytest.mark.parametrize("D", [8, 100, 512])
def test_embedding_bwd(D, pattern):
    E = _ext()
    c = C.emb_bwd_case(D, pattern)
    tokens, dy = _dev(c["tokens"], c["dy"])
    tag = f"embed bwd D={D} {pattern}"
    dw = E.embed_pe_bwd(dy, tokens, C.EMB_V)
    C.check_emb_bwd(D, pattern, dw.cpu(), tag)
    out = torch.full((C.EMB_V, D), 7.0, device="cuda", dtype=torch.bfloat16)
    r = E.embed_pe_bwd(dy, tokens, C.EMB_V, out)
    assert r.data_ptr() == out.data_ptr()
    C.check_emb_bwd(D, pattern, out.cpu(), tag + " out=")


# ---------------------------------------------------------------------------
# argmax / accuracy
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("V", C.ARGMAX_VS)
def test_argmax_accuracy_ties(V):
    E = _ext()
    c = C.argmax_case(V)
    x, = _dev(c["x"])
    got = E.argmax_lastdim(x).cpu()
    assert got.dtype == torch.int64
    assert torch.equal(got, c["ref"]), (got.tolist(), c["ref"].tolist())
    # fp32 logits are converted to bf16 inside: an fp32 copy of the same
    # values, and fp32 data whose rounding the reference repeats
    assert torch.equal(E.argmax_lastdim(x.float()).cpu(), c["ref"])
    g = torch.Generator().manual_seed(V)
    x32 = torch.randn(16, V, generator=g)
    assert torch.equal(E.argmax_lastdim(x32.cuda()).cpu(),
                       C.lowest_argmax(x32.bfloat16()))

    R = x.shape[0]
    mixed = torch.where(torch.arange(R) % 3 == 0, c["hit"], c["miss"])
    mixed[1::4] = 0                                     # pads
    for name, tg in [("hit", c["hit"]), ("miss", c["miss"]),
                     ("mixed", mixed)]:
        want = C.accuracy_ref(c["x"], tg)
        for logits in (x, x.float()):
            got = tuple(E.accuracy(logits, tg.cuda()))
            assert got == want, (V, name, logits.dtype, got, want)
    t32 = C.lowest_argmax(x32.bfloat16())
    t32[::5] = 0
    assert tuple(E.accuracy(x32.cuda(), t32.cuda())) == \
        C.accuracy_ref(x32.bfloat16(), t32)
