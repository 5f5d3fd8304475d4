"""The GEMM family against an fp64 reference, element-wise, and against exact
integer arithmetic.

gemm128_nt / gemm_nn / gemm_tn (gemm_kernel), gemm256_nt, gemm_dw,
gemm_uni_nt / _nn / _tn and the wide ragged-vocab branch of _dw_gemm, called
on the extension itself so that the dispatch heuristics cannot move a case.
Cases, reference, limits and the arm each case reaches are
tests/_gemm_cases.py; the same checks are proven on an fp32 emulation, and
the arms on a replay of the host arithmetic, in tests/test_gemm_bounds.py.

Per case: check (a) on random bf16 inputs, check (b) on integer inputs with
equality, a second call that must be bit-identical (except gemm_kernel's
split-K, whose fp32 atomics reorder the sum), and for the cases that pass
out=, a sentinel window around C.  The fp64 reference is computed on the GPU.

TR-mode operands of gemm_uni (w of nn, dy and x of tn) are [:, :n] views of
zeroed buffers whose rows run out to the next multiple of 256, so the kernel's
full-tile staging stays inside the allocation."""

import pytest
import torch

import _gemm_cases as G
from test_gpu_gemm256_store import _SENT, _window

pytestmark = pytest.mark.gpu


def _ext():
    from transformer_amd.ops import ext
    return ext()


def _padded(t):
    """t as the [:, :n] view of a zeroed (rows, n rounded up to 256) buffer
    that it starts at the beginning of: the storage covers every row's pad."""
    rows, n = t.shape
    ld = (n + 255) // 256 * 256
    full = torch.zeros(rows, ld, device="cuda", dtype=torch.bfloat16)
    full[:, :n] = t
    v = full[:, :n]
    assert v.stride() == (ld, 1) and v.storage_offset() == 0
    assert v.untyped_storage().nbytes() >= 2 * rows * ld
    return v


def _operands(c, L, R, bias):
    """The kernel's own operand layout of the canonical (L, R, bias)."""
    k = c["kernel"]
    b = bias if bias is not None else torch.Tensor()
    if k in ("gemm128_nt", "gemm256_nt"):
        return (L.contiguous(), R.t().contiguous(), b)
    if k == "gemm_nn":
        return (L.contiguous(), R.contiguous())
    if k == "gemm_tn":
        return (L.t().contiguous(), R.contiguous())
    if k == "gemm_dw":
        return (L.t().contiguous(), R.contiguous())
    if k == "uni_nt":
        a = L.contiguous()
        if c["a_wide"]:
            buf = torch.zeros(L.shape[0], c["a_wide"], device="cuda",
                              dtype=torch.bfloat16)
            buf[:, :L.shape[1]] = L
            a = buf[:, :L.shape[1]]
            assert a.stride(0) > L.shape[1]
        return (a, R.t().contiguous(), bias)
    if k == "uni_nn":
        return (L.contiguous(), _padded(R))
    if k == "uni_tn":
        return (_padded(L.t()), _padded(R))
    assert k == "dw_gemm"
    dy = _padded(L.t())
    assert tuple(dy.shape) == (192, 8194) and dy.stride(0) == 8448
    return (dy, R.contiguous())


def _call(c, ops, out=None, db=None):
    E, k = _ext(), c["kernel"]
    if k == "gemm128_nt":
        return E.gemm128_nt(*ops, c["epi"], out)
    if k == "gemm256_nt":
        return E.gemm256_nt(*ops, c["epi"], out, None)
    if k == "gemm_nn":
        return E.gemm_nn(*ops, out)
    if k == "gemm_tn":
        return E.gemm_tn(*ops, out)
    if k == "gemm_dw":
        return E.gemm_dw(*ops, out, db)
    if k == "uni_nt":
        return E.gemm_uni_nt(*ops, c["epi"], out)
    if k == "uni_nn":
        return E.gemm_uni_nn(*ops, out)
    if k == "uni_tn":
        return E.gemm_uni_tn(*ops, out, c["splitr"])
    from transformer_amd.ops.gemm_dispatch import _dw_gemm
    return _dw_gemm(*ops, out=out)


def _i16(t):
    return t.view(torch.int16)


def _one_kind(c, kind):
    name = c["name"]
    M, N = c["M"], c["N"]
    L, R, bias = (t.cuda() if t is not None else None
                  for t in G.make_inputs(c, kind))
    ref = G.reference(L, R, bias)       # fp64, once, on the GPU
    ops = _operands(c, L, R, bias)
    db = torch.full((M,), float("nan"), device="cuda",
                    dtype=torch.bfloat16) if c["db"] else None
    tag = f"gpu {name} {kind}"
    if not c["out"]:
        got = _call(c, ops, None, db)
        assert tuple(got.shape) == (M, N) and got.dtype == torch.bfloat16
        assert got.is_contiguous()
    else:
        # C as a window inside a sentinel-filled buffer
        flat, start, win = _window(M, N, 0)
        r = _call(c, ops, win, db)
        torch.cuda.synchronize()
        assert r.data_ptr() == win.data_ptr()
        assert bool((flat[:start] == _SENT).all()), f"{tag}: wrote before C"
        assert bool((flat[start + M * N:] == _SENT).all()), \
            f"{tag}: wrote past C"
        inside = flat[start:start + M * N].view(M, N)
        assert bool((inside != _SENT).all()), f"{tag}: element unwritten"
        got = win
        plain = _call(c, ops, None,
                      torch.empty_like(db) if db is not None else None)
        if G.deterministic(c) or kind == "int":     # integer sums are exact
            assert torch.equal(_i16(win), _i16(plain)), \
                f"{tag}: out= differs from the returned result"
        else:
            G.check(kind, plain, L, R, bias, c["epi"], tag + " no-out", ref)
    G.check(kind, got, L, R, bias, c["epi"], tag, ref)
    if c["db"]:
        G.check_db(kind, db, L, tag)
    if G.deterministic(c):
        again = _call(c, ops, None,
                      torch.empty_like(db) if db is not None else None)
        assert torch.equal(_i16(again), _i16(got)), \
            f"{tag}: second call differs"


@pytest.mark.parametrize("name", [n for n in G.CASES
                                  if G.case(n)["kernel"] != "dw_gemm"])
def test_gemm_elementwise(name):
    c = G.case(name)
    _one_kind(c, "rand")
    _one_kind(c, "int")


@pytest.mark.parametrize("name", [n for n in G.CASES
                                  if G.case(n)["kernel"] == "dw_gemm"])
def test_dw_gemm_wide_ragged_vocab(name, monkeypatch):
    """_dw_gemm on dy (192, 8194 of 8448): the 256-aligned main span with
    splitr 1, then the 2-column tail with splitr 64; all 8194 rows of dW."""
    c = G.case(name)
    E = _ext()
    real, calls = E.gemm_uni_tn, []

    def spy(dy, x, out=None, splitr=1):
        calls.append((tuple(dy.shape), dy.stride(0), tuple(out.shape),
                      splitr))
        return real(dy, x, out, splitr)
    monkeypatch.setattr(E, "gemm_uni_tn", spy)
    for kind in ("rand", "int"):
        del calls[:]
        _one_kind(c, kind)
        per_run = [((192, 8192), 8448, (8192, 128), 1),
                   ((192, 2), 8448, (2, 128), 64)]
        assert calls and len(calls) % 2 == 0
        assert all(calls[i:i + 2] == per_run for i in range(0, len(calls), 2))


def test_unpadded_ragged_tr_operand_raises():
    """The host checks are the guard against staging past an allocation: a
    ragged TR operand whose rows do not run out to the tile is refused
    before anything is launched."""
    E = _ext()
    z = lambda *s: torch.zeros(*s, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(RuntimeError, match="not padded to the tile"):
        E.gemm_uni_tn(z(128, 300), z(128, 256), None, 1)
    with pytest.raises(RuntimeError, match="not padded to the tile"):
        E.gemm_uni_tn(z(128, 512), z(128, 200), None, 1)
    with pytest.raises(RuntimeError, match="not padded to the tile"):
        E.gemm_uni_nn(z(300, 192), z(192, 200), None)
    with pytest.raises(RuntimeError, match="not padded to the tile"):
        E.gemm_uni_nn(z(300, 192), z(192, 208)[:, :200], None)
