"""Row-streaming column sums (`colsum`), `relu_bwd_db` on the same kernel,
and the bias gradients that go through them in autograd.

Reference: the fp64 column sum of the bf16 inputs.  Bound, element-wise:
e = M * 2^-24 * sum|a| covers any fp32 summation order of M terms (to first
order), and lim = e + U * (|ref| + e) adds the one bf16 rounding of the
computed sum.  Every arm is held to it: `TFMX_COLSUM=rows` (the row kernel
wherever its 16-byte loads are possible), `TFMX_COLSUM=cols` (the column
kernel) and the unset default (the row kernel from N = 512 up)."""

import pytest
import torch

from _gpu_bounds import U, _check_lim, _env

pytestmark = pytest.mark.gpu

ARMS = {"default": None, "rows": "rows", "cols": "cols"}


def _ext():
    from transformer_amd.ops import ext
    return ext()


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _rand(g, *shape):
    """randn + 0.25: column sums that are not pure cancellation."""
    return (torch.randn(*shape, device="cuda", generator=g) + 0.25).bfloat16()


def _check_colsum(got, a, name):
    M = a.shape[0]
    a64 = a.double()
    ref = a64.sum(0)
    e = M * 2.0 ** -24 * a64.abs().sum(0)
    _check_lim(got, ref, e + U * (ref.abs() + e), name)


def _colsum(a, arm, out=None):
    with _env(TFMX_COLSUM=ARMS[arm]):
        return _ext().colsum(a, out)


def _dense(M, N, lda, seed):
    """(M, N) view with row stride lda of a zero-padded (M, lda) buffer."""
    buf = torch.zeros(M, lda, device="cuda", dtype=torch.bfloat16)
    buf[:, :N] = _rand(_gen(seed), M, N)
    return buf[:, :N]


_SHAPES = [
    (1, 8, 8),
    (63, 8, 8),
    (64, 512, 512),       # one row group, 8 rows per wave
    (257, 520, 520),      # ragged last chunk, odd row count
    (300, 1536, 1536),
    (129, 2048, 2048),    # four panels, two row groups (129 > 128 rows)
    (130, 4104, 4104),    # two-chunk panels, N not a multiple of 512
    (40, 8712, 8712),     # four-chunk panels
    (200, 1026, 1280),    # guarded tail group inside a padded row
]


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("M,N,lda", _SHAPES)
def test_colsum(M, N, lda, arm):
    a = _dense(M, N, lda, seed=M + N)
    assert a.stride(0) == lda and a.data_ptr() % 16 == 0
    _check_colsum(_colsum(a, arm), a, f"colsum {arm} {M}x{N} lda={lda}")


@pytest.mark.parametrize("arm", list(ARMS))
def test_colsum_read_bound(arm):
    """The input ends at element (M-1)*lda + N - 1: the allocation is exactly
    that long, and the pad columns of the rows before the last hold NaN, so
    a tail group read as a whole would poison a sum."""
    M, N, lda = 200, 1026, 1280
    buf = torch.full(((M - 1) * lda + N,), float("nan"), device="cuda",
                     dtype=torch.bfloat16)
    a = buf.as_strided((M, N), (lda, 1))
    a.copy_(_rand(_gen(7), M, N))
    assert buf.numel() == (M - 1) * lda + N and a.data_ptr() % 16 == 0
    _check_colsum(_colsum(a, arm), a, f"colsum {arm} exact allocation")


@pytest.mark.parametrize("arm", list(ARMS))
def test_colsum_fallback_shapes(arm):
    """Row stride not a multiple of 8, and a view that starts one element
    into its buffer: no 16-byte loads possible, the column kernel runs."""
    a = _dense(100, 33, 33, seed=1)
    _check_colsum(_colsum(a, arm), a, f"colsum {arm} 100x33")
    buf = torch.zeros(100 * 64 + 1, device="cuda", dtype=torch.bfloat16)
    b = buf[1:].view(100, 64)
    b.copy_(_rand(_gen(2), 100, 64))
    assert b.data_ptr() % 16 == 2
    _check_colsum(_colsum(b, arm), b, f"colsum {arm} offset view")


@pytest.mark.parametrize("arm", list(ARMS))
def test_colsum_exact(arm):
    """All-equal inputs: every partial sum is a multiple of 0.5 below 2^8,
    exact in fp32 in any order, and the total 128 is a bf16 number."""
    a = torch.full((256, 520), 0.5, device="cuda", dtype=torch.bfloat16)
    got = _colsum(a, arm)
    assert torch.equal(got.float(), torch.full_like(got, 128.0).float())


def test_colsum_workspace_repeated():
    """15 back-to-back calls on the one cached workspace of N = 512,
    alternating the row count (so the grid) and the arm: a counter or a
    re-zero that is wrong for a changed grid shows in the next result."""
    g = _gen(11)
    cases = [(_rand(g, (64, 257, 4096)[it % 3], 512),
              "cols" if it % 2 else "rows") for it in range(15)]
    outs = [_colsum(a, arm) for a, arm in cases]   # no sync in between
    torch.cuda.synchronize()
    for it, ((a, arm), out) in enumerate(zip(cases, outs)):
        _check_colsum(out, a, f"repeat it={it} {arm} M={a.shape[0]}")


def test_colsum_out_argument():
    a = _dense(300, 1536, 1536, seed=3)
    out = torch.empty(1536, device="cuda", dtype=torch.bfloat16)
    got = _colsum(a, "rows", out)
    assert got.data_ptr() == out.data_ptr()
    _check_colsum(out, a, "colsum out=")


# ---------------------------------------------------------------------------
# relu_bwd_db
# ---------------------------------------------------------------------------

# +0.0, -0.0, NaN, +inf, -inf, smallest positive / negative subnormal
_SPECIAL_BITS = [0x0000, -0x8000, 0x7FC0, 0x7F80, -0x0080, 0x0001, -0x7FFF]


def _relu_inputs(M, N):
    g = _gen(M * 31 + N)
    dy = _rand(g, M, N)
    y = torch.randn(M, N, device="cuda", generator=g).bfloat16()
    bits = torch.tensor(_SPECIAL_BITS, device="cuda", dtype=torch.int16)
    y.view(-1).view(torch.int16)[:bits.numel()] = bits
    return dy, y


@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("M,N", [
    (1, 8), (257, 520), (129, 2048),
    (300, 33),                 # N % 8 != 0: relu_bwd + colsum
    (40, 4104), (40, 8712),    # two- and four-chunk panels
])
def test_relu_bwd_db(M, N, arm):
    E = _ext()
    dy, y = _relu_inputs(M, N)
    db_out = torch.empty(N, device="cuda", dtype=torch.bfloat16)
    with _env(TFMX_COLSUM=ARMS[arm]):
        dz, db = E.relu_bwd_db(dy, y, db_out)
    ref_dz = E.relu_bwd(dy, y)
    assert torch.equal(dz.view(torch.int16), ref_dz.view(torch.int16))
    # the special values: kept for +inf and the positive subnormal only
    keep = torch.tensor([0, 0, 0, 1, 0, 1, 0], device="cuda", dtype=torch.bool)
    flat_dz, flat_dy = dz.view(-1)[:7], dy.view(-1)[:7]
    assert torch.equal(flat_dz, torch.where(keep, flat_dy,
                                            torch.zeros_like(flat_dy)))
    assert db.data_ptr() == db_out.data_ptr()
    _check_colsum(db_out, dz, f"relu_bwd_db {arm} {M}x{N}")


def test_relu_bwd_db_fresh_output():
    dy, y = _relu_inputs(257, 520)
    dz, db = _ext().relu_bwd_db(dy, y)
    assert db.shape == (520,) and db.dtype == torch.bfloat16
    _check_colsum(db, dz, "relu_bwd_db db=None")


# ---------------------------------------------------------------------------
# autograd: the bias gradient of a relu linear and of the FFN composite
# ---------------------------------------------------------------------------

def _spy_first_arg(monkeypatch, name, seen):
    """Record the dY handed to functional.<name> (the dW GEMM's input: dz)."""
    from transformer_amd.ops import functional as F
    orig = getattr(F, name)

    def spy(dy, *a, **k):
        seen.append(dy)
        return orig(dy, *a, **k)
    monkeypatch.setattr(F, name, spy)


def _backward(y, dy, leaves, arm):
    for t in leaves.values():
        t.grad = None
    with _env(TFMX_COLSUM=ARMS[arm], TFMX_FFN_BWD=None, TFMX_LN_BWD=None):
        y.backward(dy, retain_graph=True)
    torch.cuda.synchronize()
    return {n: t.grad.clone() for n, t in leaves.items()}


@pytest.mark.parametrize("bias", [True, False])
def test_linear_relu_bias_grad(bias, monkeypatch):
    import transformer_amd.ops as ops
    M, K, N = 2048, 128, 128
    g = _gen(21)
    x = torch.randn(M, K, device="cuda", generator=g).bfloat16() \
        .requires_grad_()
    w = (torch.randn(N, K, device="cuda", generator=g) * K ** -0.5) \
        .bfloat16().requires_grad_()
    leaves = {"x": x, "w": w}
    if bias:
        leaves["b"] = (torch.randn(N, device="cuda", generator=g) * 0.1) \
            .bfloat16().requires_grad_()
    dy = _rand(g, M, N)
    seen = []
    _spy_first_arg(monkeypatch, "_dw_db_gemm", seen)
    y = ops.linear(x, w, leaves.get("b"), activation="relu")
    got = _backward(y, dy, leaves, "default")
    ref = _backward(y, dy, leaves, "cols")
    dz_rows, dz_cols = seen
    assert torch.equal(dz_rows, dz_cols), "dz differs between the arms"
    assert torch.equal(dz_rows, _ext().relu_bwd(dy, y.detach()))
    assert torch.equal(got["w"], ref["w"]), "dW differs between the arms"
    assert torch.equal(got["x"], ref["x"]), "dX differs between the arms"
    if bias:
        _check_colsum(got["b"], dz_rows, "linear relu db rows")
        _check_colsum(ref["b"], dz_cols, "linear relu db cols")


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("M", [4096, 8192])
def test_ffn_block_bias_grad(M, flat, monkeypatch):
    """FFN composite, default arm: b1.grad is the column sum of the dz that
    the arm produced, and dz, dW1, dW2 are bit-equal to a backward with
    TFMX_COLSUM=cols.  dX is bit-equal at M = 8192, where both dX GEMMs run
    on the deterministic gemm256 kernel.  At M = 4096 the final dX GEMM
    (N = 512) runs on the 128-tile split-K kernel, whose fp32 atomics order
    moves rn(acc) by up to one ulp between ANY two backwards
    (test_gpu_fused_backward.py::test_ffn_block_arms): there dX is held to
    that kernel's own pair bound, 2u * (|acc| + |dx|), with acc the GEMM
    result before the residual add, while its input dz is bit-equal; a
    repeat of the same arm is compared the same way."""
    from transformer_amd.ops import functional as F
    E = _ext()
    d, dff = 512, 2048
    g = _gen(5)

    def rn(*s, scale=1.0):
        return (torch.randn(*s, device="cuda", generator=g) * scale) \
            .bfloat16().requires_grad_()
    params = {"w1": rn(dff, d, scale=d ** -0.5), "b1": rn(dff, scale=0.1),
              "w2": rn(d, dff, scale=dff ** -0.5), "b2": rn(d, scale=0.1),
              "gamma": rn(d), "beta": rn(d, scale=0.1)}
    if flat:
        for p in params.values():
            p._flat_grad = torch.zeros_like(p)
    x = rn(M, d)
    dy = torch.randn(M, d, device="cuda", generator=g).bfloat16()

    seen, accs = [], []
    _spy_first_arg(monkeypatch, "_dw_gemm", seen)
    orig = F._dx_gemm

    def dx_spy(E_, dyy, w):
        out = orig(E_, dyy, w)
        accs.append(out)
        return out
    monkeypatch.setattr(F, "_dx_gemm", dx_spy)

    torch.manual_seed(9)
    y = F.ffn_dropout_residual_layernorm(
        x, params["w1"], params["b1"], params["w2"], params["b2"],
        params["gamma"], params["beta"], 0.1, True)

    def run(arm):
        del seen[:], accs[:]
        if flat:
            for p in params.values():
                p._flat_grad.zero_()
        grads = _backward(y, dy, {"x": x} if flat else {"x": x, **params},
                          arm)
        if flat:
            grads.update({n: p._flat_grad.clone() for n, p in params.items()})
        assert len(seen) == 2 and len(accs) == 2   # dW2's dxm, dW1's dz
        return grads, seen[1], accs[1].float()
    got, dz_rows, acc = run("default")
    again, dz_again, _ = run("default")
    ref, dz_cols, _ = run("cols")
    assert torch.equal(dz_rows, dz_again)
    assert torch.equal(dz_rows, dz_cols), "dz differs between the arms"
    for n in ("w1", "w2"):
        assert torch.equal(got[n], ref[n]), f"d{n} differs between the arms"
    if E.gemm256_viable(M, d, dff):
        assert torch.equal(got["x"], ref["x"]), "dX differs between the arms"
    else:
        # the same arm twice is held to the same bound: the looseness is
        # the split-K GEMM's, not the arm's
        a = got["x"].float()
        for name, other in (("cols", ref), ("rows again", again)):
            b = other["x"].float()
            lim = 2 * 1.01 * U * (acc.abs() + b.abs())
            print(f"dX rows vs {name}: {int((a != b).sum())} of {a.numel()} "
                  "elements differ")
            assert bool(((a - b).abs() <= lim).all()), \
                f"dX vs {name} outside the pair bound"
    _check_colsum(got["b1"], dz_rows, f"ffn b1.grad rows M={M}")
    _check_colsum(ref["b1"], dz_cols, f"ffn b1.grad cols M={M}")
