"""gemm256 epilogue store arms (gemm256.hip, TFMX_G256_EPI, read per call).

The default epilogue swaps the MFMA operand roles so that a lane owns four
consecutive columns of one row, and stores 8 or 16 bytes per instruction
(vec8 / lds); `scalar` is the original operand order with one 2-byte store
per instruction.  The change moves bytes and leaves every K-ordered dot
product alone, so each arm must equal the scalar arm bit for bit; the
scalar arm's own values are held to an fp64 reference with the element-wise
bound of _gpu_bounds._check (u*|ref| + 1e-5 * sum|terms|).

Tile per shape, from gemm256_tile's arithmetic (replayed on the CPU by
test_tile_choice below): with g22 = ceil(M/256)*ceil(N/256) and
g21 = ceil(M/256)*ceil(N/128),

    (256, 256)     g22=1,   g21=2    -> 128x128
    (300, 384)     g22=4,   g21=6    -> 128x128, ragged M
    (4096, 1792)   g22=112, g21=224  -> 256x128
    (4096, 3584)   g22=224 (util .875 = g21's) -> 256x256
    (4000, 1800)   g22=128, g21=240  -> 256x128; last M tile 160 rows, last
                                        N tile 8 columns, N % 8 == 0
    (4080, 1794)   g22=128, g21=240  -> 256x128; even N: 4-byte pair path
    (4080, 1795)   g22=128, g21=240  -> 256x128; odd N: scalar path
    (4000, 3592)   g22=240 (util .94 > g21's .91) -> 256x256, ragged M and N
    (4000, 3590)   same tile, even N: pair path on the 256x256 instance
    (300, 382), (300, 383)  128x128, pair / scalar path

The last four are additions to the issue's seven so that the narrow paths
and ragged N also run on the 256x256 and 128x128 instances.
"""

import pytest
import torch

from _gpu_bounds import _check, _env

ARMS = ("vec8", "lds", None)     # None: the default arm

SHAPES = [
    (256, 256, 128),
    (300, 384, 128),
    (4096, 1792, 128),
    (4096, 3584, 128),
    (4000, 1800, 128),
    (4080, 1794, 128),
    (4080, 1795, 128),
    (4000, 3592, 128),
    (4000, 3590, 128),
    (300, 382, 128),
    (300, 383, 128),
]
RAGGED = [s for s in SHAPES if s[0] % 256 or s[1] % 128]

_TILES = {
    (256, 256): (128, 128), (300, 384): (128, 128),
    (4096, 1792): (256, 128), (4096, 3584): (256, 256),
    (4000, 1800): (256, 128), (4080, 1794): (256, 128),
    (4080, 1795): (256, 128), (4000, 3592): (256, 256),
    (4000, 3590): (256, 256), (300, 382): (128, 128),
    (300, 383): (128, 128),
}


def _tile(m, n):
    """gemm256_tile (gemm256.hip), line for line."""
    cd = lambda a, b: (a + b - 1) // b
    g22 = cd(m, 256) * cd(n, 256)
    g21 = cd(m, 256) * cd(n, 128)
    util = lambda g: 0.0 if g < 1 else g / ((g + 255) // 256 * 256)
    if g22 >= 224:
        return (256, 128) if util(g21) > util(g22) + 0.1 else (256, 256)
    if g21 >= 224:
        return (256, 128)
    return (128, 128)


def test_tile_choice():
    for (m, n, k) in SHAPES:
        assert _tile(m, n) == _TILES[(m, n)], (m, n)
        assert k % 64 == 0 and k >= 128
    assert {_TILES[(m, n)] for m, n, _ in SHAPES} == \
        {(128, 128), (256, 128), (256, 256)}


def _ext():
    from transformer_amd.ops import ext
    return ext()


def _inputs(m, n, k):
    g = torch.Generator(device="cuda").manual_seed(7 * m + n)
    a = torch.randn(m, k, device="cuda", generator=g).bfloat16()
    w = torch.randn(n, k, device="cuda", generator=g).bfloat16()
    bias = torch.randn(n, device="cuda", generator=g).bfloat16()
    aux = torch.randn(m, n, device="cuda", generator=g).bfloat16()
    flat = aux.view(-1)
    flat[0::7] = 0.0
    flat[3::11] = -0.0
    assert bool((flat < 0).any()) and bool((flat == 0).any())
    assert bool((flat.view(torch.int16) == -32768).any()), "no -0.0 in aux"
    return a, w, bias, aux


def _runs(a, w, bias, aux):
    """{name: gemm256_nt arguments after (a, w)}"""
    nob = torch.Tensor()
    return {
        "plain": (nob, 0, None, None),
        "bias": (bias, 0, None, None),
        "bias_relu": (bias, 1, None, None),
        "relu_mask": (nob, 2, None, aux),
        "res_add": (nob, 3, None, aux),
    }


def _i16(t):
    return t.view(torch.int16)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", SHAPES)
def test_store_arms(m, n, k):
    E = _ext()
    a, w, bias, aux = _inputs(m, n, k)
    runs = _runs(a, w, bias, aux)
    with _env(TFMX_G256_EPI="scalar"):
        old = {name: E.gemm256_nt(a, w, *args) for name, args in runs.items()}
    for arm in ARMS:
        with _env(TFMX_G256_EPI=arm):
            for name, args in runs.items():
                got = E.gemm256_nt(a, w, *args)
                assert torch.equal(_i16(got), _i16(old[name])), \
                    f"{name} {m}x{n}x{k}: arm {arm} differs from scalar"
            out = torch.empty(m, n, device="cuda", dtype=torch.bfloat16)
            r = E.gemm256_nt(a, w, bias, 1, out, None)
            assert r.data_ptr() == out.data_ptr()
            assert torch.equal(_i16(out), _i16(old["bias_relu"])), \
                f"out= {m}x{n}x{k}: arm {arm} differs from scalar"

    # fp64 reference for what all the arms agreed on
    ad, wd = a.double(), w.double()
    prod = ad @ wd.T
    absp = (ad.abs() @ wd.abs().T).float()
    bd, xd = bias.double(), aux.double()
    tag = f"{m}x{n}x{k}"
    _check(old["plain"], prod, absp, f"plain {tag}")
    _check(old["bias"], prod + bd, absp + bd.abs().float(), f"bias {tag}")
    _check(old["bias_relu"], (prod + bd).clamp(min=0),
           absp + bd.abs().float(), f"bias_relu {tag}")
    _check(old["relu_mask"], torch.where(xd > 0, prod, torch.zeros_like(prod)),
           absp, f"relu_mask {tag}")
    assert bool((old["relu_mask"][aux <= 0] == 0).all())
    _check(old["res_add"], prod + xd, absp + xd.abs().float(),
           f"res_add {tag}")


_SENT = 0x7FC1   # a NaN payload no finite-input GEMM writes


def _window(m, n, off):
    """(flat sentinel buffer, its (m, n) window starting `off` elements in)"""
    pad = 4096
    flat = torch.full((pad + m * n + pad,), _SENT, device="cuda",
                      dtype=torch.int16)
    start = pad + off
    return flat, start, flat[start:start + m * n].view(torch.bfloat16) \
        .view(m, n)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 1, 2])
@pytest.mark.parametrize("m,n,k", RAGGED)
def test_store_guards(m, n, k, off):
    """C is an (m, n) window `off` elements into a sentinel-filled buffer:
    nothing outside the window may change, everything inside must be
    written (and equal the scalar arm, so a store that ran past column n
    into the next row shows too).  off = 0 keeps the window 16-byte
    aligned; off = 2 / 1 leave it 4- / 2-byte aligned, which must send the
    call down the pair / scalar path whatever n is."""
    E = _ext()
    a, w, bias, aux = _inputs(m, n, k)
    with _env(TFMX_G256_EPI="scalar"):
        ref = {e: E.gemm256_nt(a, w, bias if e < 2 else torch.Tensor(), e,
                               None, aux if e >= 2 else None)
               for e in (1, 2, 3)}
    for arm in ARMS:
        for e in (1, 2, 3):
            flat, start, out = _window(m, n, off)
            assert out.data_ptr() % 16 == (2 * off) % 16
            with _env(TFMX_G256_EPI=arm):
                E.gemm256_nt(a, w, bias if e < 2 else torch.Tensor(), e, out,
                             aux if e >= 2 else None)
            torch.cuda.synchronize()
            tag = f"{m}x{n}x{k} off={off} arm={arm} epi={e}"
            assert bool((flat[:start] == _SENT).all()), f"{tag}: wrote before C"
            assert bool((flat[start + m * n:] == _SENT).all()), \
                f"{tag}: wrote past C"
            inside = flat[start:start + m * n].view(m, n)
            assert bool((inside[-1] != _SENT).all()), f"{tag}: last row unwritten"
            assert bool((inside[:, -1] != _SENT).all()), \
                f"{tag}: last column unwritten"
            assert bool((inside != _SENT).all()), f"{tag}: element unwritten"
            assert torch.equal(inside, _i16(ref[e])), f"{tag}: differs"


@pytest.mark.gpu
def test_unaligned_aux_and_bias():
    """aux 4-byte aligned / bias 2-byte aligned with N % 8 == 0: the host
    check must drop to the narrow paths, not issue misaligned wide loads."""
    E = _ext()
    m, n, k = 4000, 1800, 128
    a, w, bias, aux = _inputs(m, n, k)
    auxbuf = torch.empty(m * n + 8, device="cuda", dtype=torch.bfloat16)
    aux2 = auxbuf[2:2 + m * n].view(m, n)
    aux2.copy_(aux)
    biasbuf = torch.empty(n + 8, device="cuda", dtype=torch.bfloat16)
    bias1 = biasbuf[1:1 + n]
    bias1.copy_(bias)
    nob = torch.Tensor()
    with _env(TFMX_G256_EPI="scalar"):
        r2 = E.gemm256_nt(a, w, nob, 2, None, aux)
        r3 = E.gemm256_nt(a, w, nob, 3, None, aux)
        r1 = E.gemm256_nt(a, w, bias, 1, None, None)
    for arm in ARMS:
        with _env(TFMX_G256_EPI=arm):
            assert torch.equal(_i16(E.gemm256_nt(a, w, nob, 2, None, aux2)),
                               _i16(r2)), arm
            assert torch.equal(_i16(E.gemm256_nt(a, w, nob, 3, None, aux2)),
                               _i16(r3)), arm
            assert torch.equal(_i16(E.gemm256_nt(a, w, bias1, 1, None, None)),
                               _i16(r1)), arm


@pytest.mark.gpu
def test_special_values():
    """Outputs in the fp32-denormal range, overflow to inf, NaN / inf
    inputs and signed zeros: the arms share the scalar arm's integer
    rounding, so they agree bit for bit here too (a hardware convert would
    quiet the NaNs differently)."""
    E = _ext()
    m, n, k = 4096, 1792, 128
    g = torch.Generator(device="cuda").manual_seed(11)
    fa = torch.randn(m, k, device="cuda", generator=g)
    fw = torch.randn(n, k, device="cuda", generator=g)
    nob = torch.Tensor()
    cases = [((fa * sa).bfloat16(), (fw * sw).bfloat16())
             for sa, sw in ((1e-19, 1e-20), (1e-19, 1e-21), (1e19, 1e19))]
    z = fa.bfloat16().clone()
    z[::5] = 0
    zw = fw.bfloat16().clone()
    zw[::3] = -0.0
    cases += [(z, zw), (-z, zw)]
    sp = fa.bfloat16().clone()
    sp[7, 3] = float("nan")
    sp[9, 5] = float("inf")
    sp[11, 5] = float("-inf")
    cases.append((sp, fw.bfloat16()))
    for i, (a, w) in enumerate(cases):
        with _env(TFMX_G256_EPI="scalar"):
            ref = E.gemm256_nt(a, w, nob, 0)
        for arm in ARMS:
            with _env(TFMX_G256_EPI=arm):
                got = E.gemm256_nt(a, w, nob, 0)
            assert torch.equal(_i16(got), _i16(ref)), (i, arm)
