"""The bounds of tests/test_gpu_row_kernels.py, checked without a GPU.

For every bound the same inputs go through a plain fp32 torch emulation of
the kernel (its order of operations where that matters: one-pass variance,
y from the bf16-rounded s, gradient exp(x - lse32)), rounded to bf16 where
the kernel rounds, and the result must pass the SAME check function against
the fp64 reference: a bound that correct fp32 arithmetic cannot meet fails
here.  The negative cases perturb the emulation the way a subtly wrong
kernel would be wrong and must make the check fail: the checks bite.

The dropout stream oracle (numpy) is pinned against a big-integer
evaluation of the hash and must meet its statistical conditions."""

import numpy as np
import pytest
import torch

import _row_cases as C
from _gpu_bounds import (dropout_inv_keep, dropout_keep, dropout_threshold,
                         pcg_hash)


# ---------------------------------------------------------------------------
# cross entropy
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("R,V", C.CE_SHAPES)
def test_ce_bounds_admit_fp32(R, V, eps):
    tag = f"emu ce R={R} V={V} eps={eps}"
    loss, lse, full = C.ce_emulate(R, V, eps)
    C.check_ce_fwd(R, V, eps, lse, loss, tag)
    C.check_ce_grad(R, V, eps, full, 1.0, tag)
    _, _, full = C.ce_emulate(R, V, eps, dloss=2.5)
    C.check_ce_grad(R, V, eps, full, 2.5, tag + " dloss=2.5")
    # ce_fused then ce_scale: two bf16 roundings, 2u
    _, _, full = C.ce_emulate(R, V, eps)
    twice = (full.float() * 2.5).bfloat16()
    C.check_ce_grad(R, V, eps, twice, 2.5, tag + " scaled", u=2 * C.U)


@pytest.mark.parametrize("R,V", [(9, 5), (9, 1003), (300, 16)])
def test_ce_loss_formula_is_the_reference_one(R, V):
    from transformer_amd.ops import reference
    c = C.ce_case(R, V)
    for eps in (0.0, 0.1):
        want = reference.masked_cross_entropy(
            c["x"].double()[None], c["tgt"][None], C.CE_BATCH, eps)
        got = C.ce_ref(R, V, eps)["loss"]
        assert want.dtype == torch.float64
        assert abs(float(got - want)) <= 1e-12 * abs(float(want))


@pytest.mark.parametrize("perturb,eps", [("no_eps_v", 0.1),
                                         ("batch_plus_1", 0.0),
                                         ("batch_plus_1", 0.1)])
@pytest.mark.parametrize("R,V", C.CE_SHAPES)
def test_ce_checks_bite(R, V, perturb, eps):
    loss, lse, full = C.ce_emulate(R, V, eps, perturb=perturb)
    with pytest.raises(AssertionError, match="err/limit"):
        C.check_ce_grad(R, V, eps, full, 1.0, f"{perturb} V={V}")
    if perturb == "batch_plus_1":
        with pytest.raises(AssertionError, match="err/limit"):
            C.check_ce_fwd(R, V, eps, lse, loss, f"{perturb} V={V}")


def test_ce_layout_checks_bite():
    R, V = 9, 1003
    _, _, full = C.ce_emulate(R, V, 0.1)
    bad = full.clone()
    bad[3, V] = 1e-30                   # a non-zero pad column
    with pytest.raises(AssertionError, match="pad columns"):
        C.check_ce_grad(R, V, 0.1, bad, 1.0, "pad col")
    bad = full.clone()
    bad[0, 17] = -0.0                   # pad-target row: zero, but not +0
    with pytest.raises(AssertionError, match="pad rows"):
        C.check_ce_grad(R, V, 0.1, bad, 1.0, "pad row")
    with pytest.raises(AssertionError):
        C.check_ce_grad(R, V, 0.1, full[:, :V], 1.0, "unpadded")


# ---------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("R,D", C.LN_SHAPES)
def test_ln_bounds_admit_fp32(R, D):
    tag = f"emu ln R={R} D={D}"
    y, s, mean, rstd = C.ln_emulate_fwd(R, D)
    C.check_ln_fwd(R, D, y, s, mean, rstd, tag)
    C.check_ln_bwd(R, D, s, mean, rstd,
                   C.ln_emulate_bwd(R, D, s, mean, rstd), tag)


@pytest.mark.parametrize("R,D", C.LN_DROP_SHAPES)
def test_ln_dropout_bounds_admit_fp32(R, D):
    tag = f"emu ln drop R={R} D={D}"
    y, s, mean, rstd, mask = C.ln_emulate_fwd(R, D, drop=True)
    C.check_ln_fwd(R, D, y, s, mean, rstd, tag, mask=mask)
    C.check_ln_bwd(R, D, s, mean, rstd,
                   C.ln_emulate_bwd(R, D, s, mean, rstd, mask), tag,
                   mask=mask)


@pytest.mark.parametrize("R,D", C.LN_SHAPES)
def test_ln_variance_check_bites(R, D):
    """Variance over D-1: rstd is off by 1/(2(D-1)) relative."""
    y, s, mean, rstd = C.ln_emulate_fwd(R, D, perturb="var_d_minus_1")
    with pytest.raises(AssertionError, match="rstd: max err/limit"):
        C.check_ln_fwd(R, D, y, s, mean, rstd, f"var/(D-1) D={D}")


def test_ln_backward_checks_bite():
    R, D = 7, 100
    y, s, mean, rstd = C.ln_emulate_fwd(R, D)
    out = C.ln_emulate_bwd(R, D, s, mean, rstd)
    # dx without its projection on xhat
    c = C.ln_case(R, D)
    g = c["dy"].float() * c["gamma"].float()
    bad = (rstd[:, None] * (g - g.mean(-1, keepdim=True))).bfloat16()
    with pytest.raises(AssertionError, match="dx: max err/limit"):
        C.check_ln_bwd(R, D, s, mean, rstd, [bad] + out[1:], "no xhat term")
    # one row missing from the column sums
    short = (c["dy"].float()[:-1]).sum(0).bfloat16()
    with pytest.raises(AssertionError, match="dbeta: max err/limit"):
        C.check_ln_bwd(R, D, s, mean, rstd, [out[0], out[1], short],
                       "row dropped")
    # dxm kept where the mask dropped
    y, s, mean, rstd, mask = C.ln_emulate_fwd(R, D, drop=True)
    out = C.ln_emulate_bwd(R, D, s, mean, rstd, mask)
    out[3] = (out[0].float() * dropout_inv_keep(C.LN_P)).bfloat16()
    with pytest.raises(AssertionError, match="dxm at drops"):
        C.check_ln_bwd(R, D, s, mean, rstd, out, "mask ignored", mask=mask)


# ---------------------------------------------------------------------------
# dropout: the oracle itself, and that the bit checks bite
# ---------------------------------------------------------------------------

def _hash_bigint(key):
    """dropout.hip's pcg_hash in Python integers with explicit masks."""
    m64, m32 = (1 << 64) - 1, (1 << 32) - 1
    key = (key * 6364136223846793005 + 1442695040888963407) & m64
    x = ((key ^ (key >> 33)) >> 11) & m32
    x ^= x >> 16
    x = (x * 0x7feb352d) & m32
    x ^= x >> 15
    x = (x * 0x846ca68b) & m32
    x ^= x >> 16
    return x


def test_hash_oracle_matches_big_integer_arithmetic():
    keys = [0, 1, 2, 0x9E3779B97F4A7C15, (1 << 64) - 1, (1 << 63) + 12345,
            1234 * 0x9E3779B97F4A7C15 % (1 << 64)]
    got = pcg_hash(np.array(keys, dtype=np.uint64))
    assert got.dtype == np.uint32
    assert [int(v) for v in got] == [_hash_bigint(k) for k in keys]
    assert int(dropout_threshold(0.1)) == 429496736     # fp32(0.1) * 2^32
    assert int(dropout_threshold(0.5)) == 1 << 31
    assert int(dropout_threshold(0.0)) == 0
    m64 = (1 << 64) - 1
    for seed, counter in [(4321, None), (4321, 3), (-5, 4)]:
        s = seed & m64
        if counter is not None:
            s = (s * 0xD1342543DE82EF95 + counter) & m64
        want = [int(_hash_bigint((s * 0x9E3779B97F4A7C15 + i) & m64)
                    >= 429496736) for i in range(64)]
        assert dropout_keep(64, 0.1, seed, counter).tolist() == want


def test_hash_oracle_statistics():
    """p = 0.1, n = 2^20, fixed seeds: keep rate within 5 sigma of 0.9
    overall and at each position i mod 4 (the lanes of the 4-wide vector
    path); two seeds agree on p^2 + (1-p)^2 of the elements."""
    n, p = 1 << 20, 0.1
    seeds = (1234, 7, 2024)
    masks = [dropout_keep(n, p, s).astype(np.float64) for s in seeds]
    for s, m in zip(seeds, masks):
        sig = (p * (1 - p) / n) ** 0.5
        assert abs(m.mean() - (1 - p)) <= 5 * sig, (s, m.mean())
        for k in range(4):
            mk = m[k::4]
            assert abs(mk.mean() - (1 - p)) <= 5 * 2 * sig, (s, k, mk.mean())
    q = p * p + (1 - p) * (1 - p)
    sig = (q * (1 - q) / n) ** 0.5
    for a in range(3):
        for b in range(a + 1, 3):
            agree = (masks[a] == masks[b]).mean()
            assert abs(agree - q) <= 5 * sig, (seeds[a], seeds[b], agree)
    # the device-counter rule gives another stream of the same rate
    m3, m4 = (dropout_keep(n, p, 1234, k).astype(np.float64) for k in (3, 4))
    assert abs((m3 == m4).mean() - q) <= 5 * sig


@pytest.mark.parametrize("n", [4, 5, 1024, 1027])
def test_dropout_check_bites_on_swapped_vector_elements(n):
    """Two elements of one 4-vector exchanged in y (a wrong lane picked in
    the vector path) must fail the bit comparison; the right y passes."""
    p = 0.5
    c = C.dropout_case(n)
    mask = torch.from_numpy(dropout_keep(n, p, C.DROP_SEED))
    y = C.dropout_expected(c["x"], mask, p)
    dx = C.dropout_expected(c["dy"], mask, p)
    C.check_dropout(n, p, y, mask, dx, f"emu n={n}")
    yb = y.view(torch.int16)
    for v in range(0, n - 3, 4):        # a vector whose first two differ
        if yb[v] != yb[v + 1]:
            break
    else:
        pytest.fail("no vector with two different elements")
    bad = y.clone()
    bad[v], bad[v + 1] = y[v + 1], y[v]
    with pytest.raises(AssertionError, match=": y"):
        C.check_dropout(n, p, bad, mask, dx, "swapped")
    badm = mask.clone()
    badm[v], badm[v + 1] = 1 - mask[v], 1 - mask[v + 1]
    with pytest.raises(AssertionError, match="oracle"):
        C.check_dropout(n, p, y, badm, dx, "mask")


# ---------------------------------------------------------------------------
# embedding
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("D", [8, 100, 512, 520])
def test_embedding_bounds_admit_fp32(D):
    for positions in (False, True):
        C.check_emb_fwd(D, C.emb_emulate_fwd(D, positions),
                        f"emu emb D={D} pos={positions}", positions)
    with pytest.raises(AssertionError, match="err/limit"):
        C.check_emb_fwd(D, C.emb_emulate_fwd(D, False), "wrong pe", True)
    if D != 520:
        for pattern in C.EMB_BWD_PATTERNS:
            C.check_emb_bwd(D, pattern, C.emb_emulate_bwd(D, pattern),
                            f"emu emb bwd D={D} {pattern}")
        dw = C.emb_emulate_bwd(D, "same")
        dw[6, 0] = -0.0                 # within the bound, but written
        with pytest.raises(AssertionError, match="unused"):
            C.check_emb_bwd(D, "same", dw, "stray write")


# ---------------------------------------------------------------------------
# argmax
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("V", C.ARGMAX_VS)
def test_argmax_reference_and_tie_rule(V):
    c = C.argmax_case(V)
    x, ref = c["x"], c["ref"]
    assert int(ref[0]) == 0                         # all equal
    assert bool((x.float().gather(1, ref[:, None])[:, 0]
                 == x.float().max(-1).values).all())
    hi = C.highest_argmax(x)
    if V == 1:
        assert torch.equal(hi, ref)
        return
    # the highest-index rule differs on every constructed tie (bf16 rounding
    # may add ties of its own in the random rows)
    made = c["made_tie"]
    n_ties = 1 + sum(a < b < V for a, b in [(5, V - 1), (63, 64), (64, 127)])
    assert int(made.sum()) == n_ties + (V > 40)
    assert bool((ref[made] < hi[made]).all())
    assert torch.equal(c["miss"][made], hi[made])
    # accuracy targets: hits count, misses and pads do not
    R = x.shape[0]
    nz = int((ref != 0).sum())                      # a hit at 0 is a pad
    assert 0 < nz < R and C.accuracy_ref(x, c["hit"]) == (nz, nz)
    correct, total = C.accuracy_ref(x, c["miss"])
    assert correct == 0 and 0 < total <= R
    assert C.accuracy_ref(x, hi)[0] < C.accuracy_ref(x, ref)[0]
