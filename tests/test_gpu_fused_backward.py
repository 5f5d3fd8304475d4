"""One-pass LayerNorm backward with column sums, the gemm256 relu-mask /
residual-add epilogues, and the sublayer composites built on them.

References are fp32 torch on the same bf16 inputs.  Bounds are element-wise
with u = 2^-8 (bf16 unit roundoff): a bf16 result of an fp32 sum is within
u*|ref| of the exact value, plus 1e-5 * sum|terms| for the fp32 summation
order.  Two such results (the same sum taken in two orders, each rounded to
bf16) are each inside that bound, so they are compared at twice it."""

import pytest
import torch

from _gpu_bounds import U, _check, _check_pair, _env

pytestmark = pytest.mark.gpu

P = 0.3


def _ext():
    from transformer_amd.ops import ext
    return ext()


# ---------------------------------------------------------------------------
# fused ln_bwd
# ---------------------------------------------------------------------------

def _ln_case(R, D, drop, seed=0):
    E = _ext()
    g = torch.Generator(device="cuda").manual_seed(seed)

    def rn(*s):
        return torch.randn(*s, device="cuda", generator=g).bfloat16()
    x, res, dy = rn(R, D), rn(R, D), rn(R, D)
    gamma, beta = rn(D), rn(D)
    if drop:
        _, s, mean, rstd, mask = E.ln_fwd(x, res, gamma, beta, 1e-6, P, 1234,
                                          None)
    else:
        _, s, mean, rstd = E.ln_fwd(x, res, gamma, beta, 1e-6, 0.0, 0, None)
        mask = None
    return dict(dy=dy, s=s, gamma=gamma, mean=mean, rstd=rstd, mask=mask,
                D=D)


def _ln_bwd(c, arm):
    E = _ext()
    db = torch.empty(c["D"], device="cuda", dtype=torch.bfloat16) \
        if c["mask"] is not None else None
    with _env(TFMX_LN_BWD=arm):
        out = E.ln_bwd(c["dy"], c["s"], c["gamma"], c["mean"], c["rstd"],
                       None, None, c["mask"], P if db is not None else 0.0,
                       db)
    assert len(out) == (5 if db is not None else 3)
    if db is not None:
        assert out[4].data_ptr() == db.data_ptr()
    return out


def _ln_check_sums(c, out, tag):
    dyf, sf = c["dy"].float(), c["s"].float()
    xh = (sf - c["mean"][:, None]) * c["rstd"][:, None]
    tg = dyf * xh
    _check(out[1], tg.sum(0), tg.abs().sum(0), f"{tag} dgamma")
    _check(out[2], dyf.sum(0), dyf.abs().sum(0), f"{tag} dbeta")
    if c["mask"] is not None:
        dxm = out[3].float()
        _check(out[4], dxm.sum(0), dxm.abs().sum(0), f"{tag} dbias")


@pytest.mark.parametrize("drop", [False, True])
@pytest.mark.parametrize("R,D", [
    (5, 128),       # fewer rows than one block; a quarter of the wave active
    (257, 512),     # ragged last block
    (4100, 512),    # > 4096 rows: grid-stride loop runs a second pass
    (4097, 1024),   # two 512-column chunks
    (64, 100),      # D % 8 != 0: two-kernel fallback
])
def test_ln_bwd_fused(R, D, drop):
    c = _ln_case(R, D, drop)
    got = _ln_bwd(c, None)
    ref = _ln_bwd(c, "split")
    torch.cuda.synchronize()
    assert torch.equal(got[0], ref[0]), "dx differs from the split arm"
    if drop:
        assert torch.equal(got[3], ref[3]), "dxm differs from the split arm"
    _ln_check_sums(c, got, f"fused R={R} D={D} drop={drop}")
    _ln_check_sums(c, ref, f"split R={R} D={D} drop={drop}")


def test_ln_bwd_fused_repeated():
    """15 back-to-back calls, alternating R and mask/no-mask, on the one
    cached workspace: re-zeroing and the finalize's stale-L1 acquire."""
    cases = [_ln_case(2048 + 256 * (it % 3), 512, it % 2 == 0, seed=it)
             for it in range(15)]
    outs = [_ln_bwd(c, None) for c in cases]   # no sync in between
    torch.cuda.synchronize()
    for it, (c, out) in enumerate(zip(cases, outs)):
        _ln_check_sums(c, out, f"repeat it={it}")


# ---------------------------------------------------------------------------
# gemm256 epilogues
# ---------------------------------------------------------------------------

_G256_SHAPES = [
    (256, 256, 128),      # 128x128 tile
    (300, 384, 128),      # 128x128 tile, ragged M
    (4096, 1792, 128),    # 256x128 tile
    (4096, 3584, 128),    # 256x256 tile
]


def _g256_inputs(m, n, k):
    g = torch.Generator(device="cuda").manual_seed(m + n)
    a = torch.randn(m, k, device="cuda", generator=g).bfloat16()
    w = torch.randn(n, k, device="cuda", generator=g).bfloat16()
    aux = torch.randn(m, n, device="cuda", generator=g).bfloat16()
    return a, w, aux


@pytest.mark.parametrize("m,n,k", _G256_SHAPES)
def test_gemm256_relu_mask_epilogue(m, n, k):
    E = _ext()
    a, w, aux = _g256_inputs(m, n, k)
    flat = aux.view(-1)
    flat[0::7] = 0.0
    flat[3::11] = -0.0
    assert bool((flat < 0).any()) and bool((flat == 0).any())
    assert bool((flat.view(torch.int16) == -32768).any()), "no -0.0 in aux"
    nob = torch.Tensor()
    got = E.gemm256_nt(a, w, nob, 2, None, aux)
    ref = E.relu_bwd(E.gemm256_nt(a, w, nob, 0), aux)
    assert torch.equal(got.view(torch.int16), ref.view(torch.int16))


@pytest.mark.parametrize("m,n,k", _G256_SHAPES)
def test_gemm256_residual_add_epilogue(m, n, k):
    E = _ext()
    a, w, aux = _g256_inputs(m, n, k)
    got = E.gemm256_nt(a, w, torch.Tensor(), 3, None, aux)
    ref = a.float() @ w.float().T + aux.float()
    _check(got, ref, a.float().abs() @ w.float().abs().T,
           f"residual-add {m}x{n}x{k}")


# ---------------------------------------------------------------------------
# composites: default path vs the two split arms, one forward, three
# backwards over the same saved state (the arms are read per backward call)
# ---------------------------------------------------------------------------

_ARMS = {"default": {}, "ln_split": {"TFMX_LN_BWD": "split"},
         "ffn_fused": {"TFMX_FFN_BWD": "fused"}}


def _backward_arms(y, dy, inputs, params, flat, spy=None):
    """{arm: ({name: grad}, {name: ready-count})} from retained backwards."""
    from transformer_amd.ops import functional as F
    res = {}
    for arm, env in _ARMS.items():
        counts = {n: 0 for n in params}
        by_id = {id(p): n for n, p in params.items()}

        def ready(p, counts=counts, by_id=by_id):
            counts[by_id[id(p)]] += 1
        for t in list(inputs.values()) + list(params.values()):
            t.grad = None
        if flat:
            for p in params.values():
                p._flat_grad.zero_()
            F.set_grad_ready_callback(params.values(), ready)
        if spy is not None:
            spy[arm] = []
            spy["cur"] = spy[arm]
        try:
            with _env(TFMX_LN_BWD=None, TFMX_FFN_BWD=None):
                with _env(**env):
                    y.backward(dy, retain_graph=True)
        finally:
            if flat:
                F.set_grad_ready_callback(params.values(), None)
        torch.cuda.synchronize()
        grads = {n: t.grad.clone() for n, t in inputs.items()}
        for n, p in params.items():
            grads[n] = (p._flat_grad if flat else p.grad).clone()
        res[arm] = (grads, counts)
    return res


def _compare_arms(res, params, flat, loose=()):
    """Parameter vectors (bias / gamma / beta) are atomics-ordered column
    sums -> pair bound; everything else is bit-equal across arms except
    the names in `loose`, which the caller checks itself."""
    base, _ = res["default"]
    for arm in ("ln_split", "ffn_fused"):
        grads, counts = res[arm]
        for n, g in grads.items():
            if n in loose:
                continue
            if n in params and params[n].dim() == 1:
                _check_pair(base[n], g, f"{arm} {n}")
            else:
                assert torch.equal(base[n], g), f"{arm}: {n} not bit-equal"
    if flat:
        for arm, (_, counts) in res.items():
            assert all(v == 1 for v in counts.values()), (arm, counts)


def _mark_flat(params):
    for p in params.values():
        p._flat_grad = torch.zeros_like(p)


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("kind", ["encoder", "decoder"])
def test_tiny_layer_arms(kind, flat):
    from transformer_amd.models.transformer import EncoderLayer, DecoderLayer
    torch.manual_seed(3)
    d, dff, B, S = 128, 256, 2, 16
    cls = EncoderLayer if kind == "encoder" else DecoderLayer
    layer = cls(d, 4, dff, rate=0.1).to("cuda", torch.bfloat16)
    params = dict(layer.named_parameters())
    for p in params.values():          # non-trivial biases / gamma / beta
        if p.dim() == 1:
            p.data.add_(torch.randn_like(p) * 0.1)
    if flat:
        _mark_flat(params)
    x = torch.randn(B, S, d, device="cuda").bfloat16().requires_grad_()
    inputs = {"x": x}
    pad = torch.zeros(B, S, device="cuda", dtype=torch.uint8)
    if kind == "encoder":
        y = layer(x, pad, True)
    else:
        enc = torch.randn(B, S, d, device="cuda").bfloat16().requires_grad_()
        inputs["enc"] = enc
        y, _, _ = layer(x, enc, pad, pad, True)
    dy = torch.randn(B, S, d, device="cuda").bfloat16()
    res = _backward_arms(y, dy, inputs, params, flat)
    _compare_arms(res, params, flat)


@pytest.mark.parametrize("flat", [False, True])
@pytest.mark.parametrize("M", [4096, 8192])
def test_ffn_block_arms(M, flat, monkeypatch):
    """FFN block at gemm256 shapes, epilogue arm (TFMX_FFN_BWD=fused)
    against the default relu_bwd + add.  Each dX GEMM takes its epilogue
    where gemm256 is viable for it: at M=4096 only the relu-mask one (the
    N=512 GEMM underfills the chip and keeps the plain path + add), at
    M=8192 both — the fused arm then makes no _dx_gemm call at all."""
    from transformer_amd.ops import functional as F
    E = _ext()
    d, dff = 512, 2048
    assert E.gemm256_viable(M, dff, d)
    both = E.gemm256_viable(M, d, dff)
    assert both == (M == 8192)
    g = torch.Generator(device="cuda").manual_seed(5)

    def rn(*s, scale=1.0):
        return (torch.randn(*s, device="cuda", generator=g) * scale) \
            .bfloat16().requires_grad_()
    params = {"w1": rn(dff, d, scale=d ** -0.5), "b1": rn(dff, scale=0.1),
              "w2": rn(d, dff, scale=dff ** -0.5), "b2": rn(d, scale=0.1),
              "gamma": rn(d), "beta": rn(d, scale=0.1)}
    if flat:
        _mark_flat(params)
    x = rn(M, d)
    dy = torch.randn(M, d, device="cuda", generator=g).bfloat16()

    spy = {}
    orig = F._dx_gemm

    def dx_spy(E_, dyy, w):
        out = orig(E_, dyy, w)
        spy["cur"].append(out)
        return out
    monkeypatch.setattr(F, "_dx_gemm", dx_spy)

    torch.manual_seed(9)
    y = F.ffn_dropout_residual_layernorm(
        x, params["w1"], params["b1"], params["w2"], params["b2"],
        params["gamma"], params["beta"], 0.1, True)
    res = _backward_arms(y, dy, {"x": x}, params, flat, spy=spy)
    assert len(spy["default"]) == len(spy["ln_split"]) == 2
    assert len(spy["ffn_fused"]) == (0 if both else 1)
    _compare_arms(res, params, flat, loose=("x",))
    # split: dx = rn(rn(acc) + dres) against the fused rn(acc + dres).
    # fused is within u*|exact| of exact = acc + dres; split adds the
    # rounding of acc (<= u*|acc|) before its own final rounding, so the
    # pair is within u*|acc| + 2u*|exact|.  acc comes from the spy, the
    # split result stands in for |exact| (the 1.01 covers that swap).
    # Where the N=512 GEMM is not gemm256-viable every arm runs it on the
    # 128-tile split-K kernel, whose fp32 atomics order differs from call
    # to call: rn(acc) itself may then move by one ulp (<= 2u*|acc|)
    # between any two backwards, so no pair of arms is bit-equal there.
    acc = spy["default"][1].float()
    xs = {arm: res[arm][0]["x"].float() for arm in _ARMS}
    if both:
        assert torch.equal(xs["default"], xs["ln_split"])
        pairs = [("ffn_fused", "default", 1.0, 2.0)]
    else:
        pairs = [("ffn_fused", "default", 2.0, 2.0),
                 ("ln_split", "default", 2.0, 2.0)]
    for p, q, ca, cx in pairs:
        lim = 1.01 * U * (ca * acc.abs() + cx * xs[q].abs())
        err = (xs[p] - xs[q]).abs()
        worst = float((err / lim.clamp(min=1e-30)).max())
        print(f"dx {p} vs {q}: max err/limit = {worst:.4f}")
        assert bool((err <= lim).all()), (p, q, worst)
