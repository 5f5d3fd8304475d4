"""Cases, fp64 reference, element-wise limits, CPU replicas of the host
dispatch arithmetic and an fp32 emulation of the GEMM family (ops/csrc/
gemm.hip, gemm256.hip, gemm_dw.hip, gemm_uni.hip and the wide ragged dW
branch of ops/gemm_dispatch._dw_gemm).

Shared by tests/test_gpu_gemm_elementwise.py (the HIP kernels) and
tests/test_gemm_bounds.py (the emulation, on the CPU).  Plain torch; the
extension is not imported.

Every case is held in one canonical form, C[M,N] = L[M,K] @ R[K,N] (+ bias
over N) (+ ReLU); the GPU test lays L and R out the way each kernel takes its
operands (w = R^T for the NT kernels, dy = L^T for the dW kernels, zero-padded
buffers for the TR-mode operands of gemm_uni).

Two checks per case.

(a) random bf16 inputs (about 1/7 exact zeros, a few -0.0) against fp64:

      |got - ref| <= u*|ref| + c(n) * (|L| @ |R| + |bias|),   u = 2^-8
      c(n) = max(1e-5, (n + 2) * 2^-24),   n = contraction terms

    One bf16 rounding (every path rounds once, after fp32 accumulation;
    f2bfbits is round-to-nearest-even).  bf16 x bf16 products are exact in
    fp32, and a sum of n fp32 terms in any order errs, to first order, by at
    most (n - 1) * 2^-24 * sum|terms|; the +3 over n - 1 covers the bias add
    and the fp32 partials of a split contraction; 1e-5 is _gpu_bounds' floor.
    This assumes the MFMA accumulates with round-to-nearest.  C_TRUNC = True
    switches c(n) to the truncation bound (n + 2) * 2^-23; it stays False
    (profiles/gemm_elementwise_bounds.md has the measured ratios).
    With ReLU the reference is clamped, the limit is the unclamped one, and
    got == 0 is demanded wherever ref + lim < 0.

(b) integer inputs in [-3, 3], integer bias in [-8, 8], no tolerance: every
    partial sum is an integer below 2^24, exact in fp32 in any order and on
    any accumulate hardware, so got must equal fp64 -> fp32 -> bf16 (RNE)
    exactly (compared as floats: -0 == +0).
"""

import functools
import zlib

import torch

from _gpu_bounds import U, _check_lim
from test_gpu_gemm256_store import _tile as gemm256_tile

C_TRUNC = False


def c_of(n):
    return max(1e-5, (n + 2) * 2.0 ** (-23 if C_TRUNC else -24))


def cd(a, b):
    return (a + b - 1) // b


# ---------------------------------------------------------------------------
# host dispatch arithmetic, line for line
# ---------------------------------------------------------------------------

def gemm_launch_plan(M, N, K, lda, ldb, ta, tb):
    """gemm.hip gemm_launch: sk / k_per_slice, the alignment template
    arguments, and whether any block takes the glds fast path."""
    BM = BN = 128
    BK = 64
    nwg = cd(M, BM) * cd(N, BN)
    sk = 1
    if nwg < 256 and K >= 4 * BK:
        sk = min((512 + nwg - 1) // nwg, K // BK, 32)
        sk = max(sk, 1)
    k_per_slice = (cd(K, BK) + sk - 1) // sk * BK
    sk = cd(K, k_per_slice)
    ala, alb = lda % 8 == 0, ldb % 8 == 0
    glds = (not ta and not tb and ala and alb and K % BK == 0
            and M // BM > 0 and N // BN > 0)
    return dict(sk=sk, kps=k_per_slice, ala=ala, alb=alb, glds=glds)


def gemm_dw_plan(M, N, K):
    """gemm_dw.hip gemm_dw: contraction M (tokens), output (N, K)."""
    DW_BM, DW_BN, DW_BK = 64, 128, 128
    ntiles = cd(N, DW_BN) * cd(K, DW_BK)
    nslices = min((M + DW_BM - 1) // DW_BM, cd(512, ntiles))
    m_per_slice = (M + nslices - 1) // nslices
    m_per_slice = (m_per_slice + DW_BM - 1) // DW_BM * DW_BM
    nslices = (M + m_per_slice - 1) // m_per_slice
    return dict(nslices=nslices, mps=m_per_slice, ntiles=ntiles)


def gemm_uni_plan(M, N, K, splitr):
    """gemm_uni.hip gemm_uni_launch: BN and the contraction slices."""
    g22 = cd(M, 256) * cd(N, 256)
    g21 = cd(M, 256) * cd(N, 128)

    def util(nwg):
        return 0.0 if nwg < 1 else nwg / ((nwg + 255) // 256 * 256)
    BN = 256 if (g22 >= 224 and not (util(g21) > util(g22) + 0.1)) else 128
    nslices, k_per_slice = 1, K
    if splitr > 1:
        nslices = splitr
        k_per_slice = ((K // 64 + nslices - 1) // nslices) * 64
        nslices = (K + k_per_slice - 1) // k_per_slice
    return dict(BN=BN, nslices=nslices, kps=k_per_slice)


def dw_gemm_branch(rows, n, ld, kx):
    """ops/gemm_dispatch._dw_gemm on dy (rows, n) with row stride ld and x
    (rows, kx): 'main+tail', 'uni' or 'gemm_dw'; and main."""
    npad = (n + 255) // 256 * 256
    if n >= 8192 and rows % 64 == 0 and (n % 256 == 0 or ld >= npad) \
            and kx % 128 == 0:
        main = (n // 256) * 256
        if main != n and main > 0:
            return "main+tail", main
        return "uni", n
    return "gemm_dw", 0


def _slices(K, kps):
    return [(k0, min(K, k0 + kps)) for k0 in range(0, K, kps)]


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

def _case(kernel, M, N, K, arm, bias=False, epi=0, out=False, db=False,
          splitr=1, a_wide=None, tag=""):
    name = f"{kernel}-{M}x{N}x{K}" + ("-bias" if bias else "") \
        + (f"-epi{epi}" if bias or epi else "") + ("-db" if db else "") \
        + (f"-s{splitr}" if kernel == "uni_tn" else "") \
        + ("-out" if out else "") + (f"-{tag}" if tag else "")
    return dict(name=name, kernel=kernel, M=M, N=N, K=K, bias=bias, epi=epi,
                out=out, db=db, splitr=splitr, a_wide=a_wide, arm=arm)


def _g(sk, kps, ala=True, alb=True, glds=False):
    return dict(sk=sk, kps=kps, ala=ala, alb=alb, glds=glds)


def _all_cases():
    out = []
    # gemm128_nt: C[M,N] = a[M,K] @ w[N,K]^T
    for (m, n, k), arm in [
            ((128, 128, 64), _g(1, 64, glds=True)),
            ((256, 128, 512), _g(8, 64, glds=True)),
            ((100, 130, 72), _g(1, 128)),               # K tail of 8
            ((33, 17, 24), _g(1, 64)),
            ((65, 129, 70), _g(1, 128, False, False)),  # lda = ldb = 70
            ((129, 65, 321), _g(3, 128, False, False))]:  # 128 + 128 + 64+1
        for epi in (0, 1):
            out.append(_case("gemm128_nt", m, n, k, arm, bias=True, epi=epi))
    out.append(_case("gemm128_nt", 64, 96, 128, _g(1, 128)))
    # gemm_nn: C[M,N] = a[M,K] @ b[K,N]; ldb = N
    out.append(_case("gemm_nn", 100, 130, 72, _g(1, 128, True, False)))
    out.append(_case("gemm_nn", 33, 17, 24, _g(1, 64, True, False)))
    out.append(_case("gemm_nn", 128, 128, 256, _g(4, 64)))
    out.append(_case("gemm_nn", 65, 70, 321, _g(3, 128, False, False)))
    # gemm_tn: C[M,N] = a[K,M]^T @ b[K,N]; lda = M, ldb = N
    out.append(_case("gemm_tn", 130, 70, 100, _g(1, 128, False, False)))
    out.append(_case("gemm_tn", 17, 33, 50, _g(1, 64, False, False)))
    out.append(_case("gemm_tn", 128, 128, 1024, _g(16, 64)))
    out.append(_case("gemm_tn", 96, 64, 777, _g(7, 128), out=True))
    # gemm256_nt beyond two K tiles
    for (m, n, k), tile in [((300, 384, 192), (128, 128)),
                            ((256, 256, 320), (128, 128)),
                            ((4080, 1795, 192), (256, 128)),
                            ((4000, 3592, 192), (256, 256))]:
        for bias, epi in ((True, 1), (False, 0)):
            out.append(_case("gemm256_nt", m, n, k,
                             dict(tile=tile, ktiles=k // 64), bias=bias,
                             epi=epi))
    # gemm_dw: C[N,K] = dy[M,N]^T @ x[M,K]; canonical (M, N, K) = the
    # kernel's (N, K, M)
    for (mt, n, k), (ns, mps), o in [
            ((64, 130, 70), (1, 64), False),
            ((37, 130, 70), (1, 64), False),
            ((1, 17, 5), (1, 64), False),
            ((200, 130, 70), (4, 64), False),
            ((4160, 128, 128), (65, 64), False),
            ((1000, 641, 641), (8, 128), False),
            ((1000, 257, 129), (16, 64), True)]:
        for db in (False, True):
            out.append(_case("gemm_dw", n, k, mt, dict(nslices=ns, mps=mps),
                             db=db, out=o))
    # gemm_uni_nt
    for (m, n, k), bn, wide in [((300, 200, 128), 128, None),
                                ((256, 128, 320), 128, None),
                                ((300, 200, 192), 128, 256),
                                ((4096, 3584, 192), 256, None),
                                ((4000, 3592, 192), 256, None)]:
        for epi in (0, 1):
            out.append(_case("uni_nt", m, n, k,
                             dict(BN=bn, nslices=1, kps=k), bias=True,
                             epi=epi, a_wide=wide))
    # gemm_uni_nn: w (K, N) read in TR mode
    out.append(_case("uni_nn", 300, 256, 192, dict(BN=128, nslices=1, kps=192)))
    out.append(_case("uni_nn", 4000, 3584, 192,
                     dict(BN=256, nslices=1, kps=192)))
    out.append(_case("uni_nn", 300, 200, 192,
                     dict(BN=128, nslices=1, kps=192), tag="ragged"))
    # gemm_uni_tn: C[N,K] = dy[Mtok,N]^T @ x[Mtok,K], both TR mode;
    # canonical (M, N, K) = (dy columns, x columns, Mtok)
    out.append(_case("uni_tn", 300, 200, 128,
                     dict(BN=128, nslices=1, kps=128), splitr=1))
    for s, ns, kps in ((1, 1, 192), (2, 2, 128), (3, 3, 64), (64, 3, 64)):
        out.append(_case("uni_tn", 300, 200, 192,
                         dict(BN=128, nslices=ns, kps=kps), splitr=s))
    for s, ns, kps in ((1, 1, 192), (2, 2, 128)):
        out.append(_case("uni_tn", 4096, 3584, 192,
                         dict(BN=256, nslices=ns, kps=kps), splitr=s))
    out.append(_case("uni_tn", 4000, 3592, 192,
                     dict(BN=256, nslices=1, kps=192), splitr=1))
    out.append(_case("uni_tn", 300, 200, 192,
                     dict(BN=128, nslices=2, kps=128), splitr=2, out=True))
    # _dw_gemm: dy (192, 8194 of 8448), x (192, 128)
    for o in (False, True):
        out.append(_case("dw_gemm", 8194, 128, 192,
                         dict(branch="main+tail", main=8192,
                              calls=[dict(BN=128, nslices=1, kps=192),
                                     dict(BN=128, nslices=3, kps=64)]),
                         out=o))
    return out


_CASES = {c["name"]: c for c in _all_cases()}
assert len(_CASES) == len(_all_cases())
CASES = list(_CASES)

_NT, _NN, _TN = (False, False), (False, True), (True, True)


def case(name):
    return _CASES[name]


def plan(c, M=None, N=None):
    """The replayed dispatch of a case (at its own M, N unless given): the
    arm in the form of c['arm'], and 'parts', a list of (row0, row1,
    [(k0, k1) contraction slices]) over the rows of C."""
    M = c["M"] if M is None else M
    N = c["N"] if N is None else N
    K, kern = c["K"], c["kernel"]
    if kern in ("gemm128_nt", "gemm_nn", "gemm_tn"):
        lda, ldb, (ta, tb) = {"gemm128_nt": (K, K, _NT), "gemm_nn": (K, N, _NN),
                              "gemm_tn": (M, N, _TN)}[kern]
        arm = gemm_launch_plan(M, N, K, lda, ldb, ta, tb)
        return dict(arm=arm, parts=[(0, M, _slices(K, arm["kps"]))])
    if kern == "gemm256_nt":
        arm = dict(tile=gemm256_tile(M, N), ktiles=K // 64)
        return dict(arm=arm, parts=[(0, M, [(0, K)])])
    if kern == "gemm_dw":
        p = gemm_dw_plan(K, M, N)
        arm = dict(nslices=p["nslices"], mps=p["mps"])
        return dict(arm=arm, parts=[(0, M, _slices(K, p["mps"]))])
    if kern in ("uni_nt", "uni_nn", "uni_tn"):
        arm = gemm_uni_plan(M, N, K, c["splitr"])
        return dict(arm=arm, parts=[(0, M, _slices(K, arm["kps"]))])
    assert kern == "dw_gemm"
    ld = (M + 255) // 256 * 256
    branch, main = dw_gemm_branch(K, M, ld, N)
    calls = [gemm_uni_plan(main, N, K, 1), gemm_uni_plan(M - main, N, K, 64)]
    arm = dict(branch=branch, main=main, calls=calls)
    return dict(arm=arm, parts=[(0, main, _slices(K, calls[0]["kps"])),
                                (main, M, _slices(K, calls[1]["kps"]))])


def _shrink(x):
    """Output extents for the CPU emulation, which has no tiles along M and
    N: one full 256 block and the case's own ragged remainder."""
    return x if x <= 1024 else 256 + (x % 256 or 256)


def emu_plan(c):
    """plan() at the emulation's (shrunk) output extents; the contraction
    slices are those of the full shape (asserted)."""
    full = plan(c)
    if c["kernel"] == "dw_gemm":
        m = _shrink(c["M"])
        main = m // 256 * 256
        parts = [(0, main, full["parts"][0][2]), (main, m, full["parts"][1][2])]
        return m, c["N"], parts
    m, n = _shrink(c["M"]), _shrink(c["N"])
    return m, n, [(0, m, full["parts"][0][2])]


# what the new cases must reach: label -> predicate over (case, arm)
def _uni(c, kern, bn, split=None):
    a = c["arm"]
    return c["kernel"] == kern and a["BN"] == bn and \
        (split is None or (a["nslices"] > 1) == split)


def _gk(c):
    return c["kernel"] in ("gemm128_nt", "gemm_nn", "gemm_tn")


REACHED = {
    "gemm_dw_kernel<SPLIT=false, DB=false>":
        lambda c: c["kernel"] == "gemm_dw" and c["arm"]["nslices"] == 1
        and not c["db"],
    "gemm_dw_kernel<SPLIT=false, DB=true>":
        lambda c: c["kernel"] == "gemm_dw" and c["arm"]["nslices"] == 1
        and c["db"],
    "gemm_dw_kernel<SPLIT=true, DB=false>":
        lambda c: c["kernel"] == "gemm_dw" and c["arm"]["nslices"] > 1
        and not c["db"],
    "gemm_dw_kernel<SPLIT=true, DB=true>":
        lambda c: c["kernel"] == "gemm_dw" and c["arm"]["nslices"] > 1
        and c["db"],
    "gemm_dw token tail inside a single slice (M < 64)":
        lambda c: c["kernel"] == "gemm_dw" and c["arm"]["nslices"] == 1
        and c["K"] < 64,
    "gemm_dw token tail in the last slice":
        lambda c: c["kernel"] == "gemm_dw" and c["arm"]["nslices"] > 1
        and c["K"] % 64 != 0,
    "gemm_uni NTxNT BN=128": lambda c: _uni(c, "uni_nt", 128),
    "gemm_uni NTxNT BN=256": lambda c: _uni(c, "uni_nt", 256),
    "gemm_uni NTxTR BN=128": lambda c: _uni(c, "uni_nn", 128),
    "gemm_uni NTxTR BN=256": lambda c: _uni(c, "uni_nn", 256),
    "gemm_uni TRxTR BN=128 unsplit": lambda c: _uni(c, "uni_tn", 128, False),
    "gemm_uni TRxTR BN=128 split": lambda c: _uni(c, "uni_tn", 128, True),
    "gemm_uni TRxTR BN=256 unsplit": lambda c: _uni(c, "uni_tn", 256, False),
    "gemm_uni TRxTR BN=256 split": lambda c: _uni(c, "uni_tn", 256, True),
    "gemm_uni two-slot ring with 2 K tiles":
        lambda c: c["kernel"].startswith("uni") and c["arm"]["kps"] == 128,
    "gemm_uni two-slot ring with 3 K tiles":
        lambda c: c["kernel"].startswith("uni") and c["arm"]["kps"] == 192,
    "gemm_uni one K tile per slice":
        lambda c: c["kernel"] == "uni_tn" and c["arm"]["kps"] == 64,
    "_dw_gemm wide ragged vocab: main + tail":
        lambda c: c["kernel"] == "dw_gemm"
        and c["arm"]["branch"] == "main+tail",
    "gemm_kernel split-K with bias and ReLU (gemm_finalize_kernel)":
        lambda c: c["kernel"] == "gemm128_nt" and c["arm"]["sk"] > 1
        and c["bias"] and c["epi"] == 1,
    "gemm_kernel unaligned lda/ldb with split-K":
        lambda c: _gk(c) and c["arm"]["sk"] > 1
        and not c["arm"]["ala"] and not c["arm"]["alb"],
    "gemm_kernel K tail of 1":
        lambda c: _gk(c) and c["K"] % 64 == 1,
    "gemm_kernel glds fast path, unsplit":
        lambda c: _gk(c) and c["arm"]["glds"] and c["arm"]["sk"] == 1,
    "gemm_kernel glds fast path, split-K":
        lambda c: _gk(c) and c["arm"]["glds"] and c["arm"]["sk"] > 1,
    "gemm256_nt 128x128 with more than two K tiles":
        lambda c: c["kernel"] == "gemm256_nt" and c["arm"]["ktiles"] > 2
        and c["arm"]["tile"] == (128, 128),
    "gemm256_nt 256x128 with more than two K tiles":
        lambda c: c["kernel"] == "gemm256_nt" and c["arm"]["ktiles"] > 2
        and c["arm"]["tile"] == (256, 128),
    "gemm256_nt 256x256 with more than two K tiles":
        lambda c: c["kernel"] == "gemm256_nt" and c["arm"]["ktiles"] > 2
        and c["arm"]["tile"] == (256, 256),
    "gemm256_nt odd and even K tile counts":
        lambda c: c["kernel"] == "gemm256_nt" and c["arm"]["ktiles"] == 5,
}

# bit-identical on two calls: everything but gemm_kernel's split-K (fp32
# atomics change the summation order; the fp64 limit covers it)
def deterministic(c):
    return not (_gk(c) and c["arm"]["sk"] > 1)


# ---------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------

def make_inputs(c, kind, M=None, N=None):
    """CPU bf16 L (M,K), R (K,N) and bias (N) or None.  kind 'rand': randn
    with about 1/7 exact zeros and 1/64 -0.0; kind 'int': integers."""
    M = c["M"] if M is None else M
    N = c["N"] if N is None else N
    K = c["K"]
    g = torch.Generator().manual_seed(
        zlib.crc32(f"{c['name']} {kind} {M} {N}".encode()))
    if kind == "int":
        L = torch.randint(-3, 4, (M, K), generator=g)
        R = torch.randint(-3, 4, (K, N), generator=g)
        b = torch.randint(-8, 9, (N,), generator=g)
        L, R, b = L.bfloat16(), R.bfloat16(), b.bfloat16()
    else:
        assert kind == "rand"

        def rn(*shape):
            t = torch.randn(*shape, generator=g).bfloat16()
            r = torch.rand(*shape, generator=g)
            t[r < 1 / 7] = 0.0
            t[r > 1 - 1 / 64] = -0.0
            return t
        L, R, b = rn(M, K), rn(K, N), rn(N)
        if L.numel() >= 256:
            assert bool((L.view(torch.int16) == -32768).any()), "no -0.0"
            assert bool((L == 0).any()) and bool((L < 0).any())
    return L, R, (b if c["bias"] else None)


# ---------------------------------------------------------------------------
# reference and checks (on whichever device the inputs live)
# ---------------------------------------------------------------------------

def reference(L, R, bias):
    """fp64 (ref before ReLU, absterm)."""
    Ld, Rd = L.double(), R.double()
    ref, absterm = Ld @ Rd, Ld.abs() @ Rd.abs()
    if bias is not None:
        ref = ref + bias.double()
        absterm = absterm + bias.double().abs()
    return ref, absterm


def check_rand(got, L, R, bias, epi, name, ref=None):
    """Check (a).  ref: a precomputed reference(L, R, bias)."""
    ref, absterm = reference(L, R, bias) if ref is None else ref
    lim = U * ref.abs() + c_of(L.shape[1]) * absterm
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape))
    if epi == 1:
        neg = ref + lim < 0
        assert bool((got[neg] == 0).all()), f"{name}: ReLU let a negative by"
        ref = ref.clamp(min=0)
    _check_lim(got, ref, lim, name)


def expected_int(L, R, bias, epi, ref=None):
    ref, _ = reference(L, R, bias) if ref is None else ref
    assert float(ref.abs().max()) < 2 ** 24
    if epi == 1:
        ref = ref.clamp(min=0)
    return ref.float().bfloat16()


def check_int(got, L, R, bias, epi, name, ref=None):
    """Check (b)."""
    exp = expected_int(L, R, bias, epi, ref)
    assert tuple(got.shape) == tuple(exp.shape), (name, tuple(got.shape))
    bad = got.float() != exp.float()
    nbad = int(bad.sum())
    print(f"{name}: exact, {nbad} of {bad.numel()} differ")
    if nbad:
        i = bad.nonzero()[0].tolist()
        assert False, (f"{name}: {nbad} elements differ, first at {i}: got "
                       f"{float(got[tuple(i)])}, expected "
                       f"{float(exp[tuple(i)])}")
    assert torch.equal(got.float(), exp.float())


def check(kind, got, L, R, bias, epi, name, ref=None):
    (check_int if kind == "int" else check_rand)(got, L, R, bias, epi, name,
                                                 ref)


def check_db(kind, db, L, name):
    """gemm_dw's fused bias gradient: db = dy.sum(0) = L.sum(1), n = tokens."""
    Ld = L.double()
    ref, absterm = Ld.sum(1), Ld.abs().sum(1)
    if kind == "int":
        assert torch.equal(db.float(), ref.float().bfloat16().float()), \
            f"{name}: db differs"
    else:
        _check_lim(db, ref, U * ref.abs() + c_of(L.shape[1]) * absterm,
                   f"{name} db")


# ---------------------------------------------------------------------------
# fp32 emulation and its perturbations
# ---------------------------------------------------------------------------

PERTURBS = ("drop_last_k", "drop_last_tile", "drop_last_slice",
            "dup_tail_row", "bias_shift", "relu_missing", "last_row_stale",
            "last_col_stale", "transpose_4x4", "truncate")
STALE = -1.0    # "previous contents" of an unwritten row or column


@functools.lru_cache(maxsize=None)
def emu_inputs(name, kind):
    c = case(name)
    m, n, parts = emu_plan(c)
    L, R, bias = make_inputs(c, kind, m, n)
    return L, R, bias, reference(L, R, bias)


def _bf16_trunc(x):
    return (x.view(torch.int32) & -65536).view(torch.float32).bfloat16()


def emulate(name, kind, perturb=None):
    """The kernels' arithmetic in fp32 torch: 64-deep K tiles summed one
    after another in fp32, the slices of a split contraction summed in fp32,
    bias add, ReLU, one rounding to bf16.  perturb makes it wrong the way a
    subtly wrong kernel would be."""
    assert perturb is None or perturb in PERTURBS
    c = case(name)
    m, n, parts = emu_plan(c)
    L, R, bias, _ = emu_inputs(name, kind)
    Lf, Rf = L.float(), R.float()
    K = c["K"]
    kcut = K
    if perturb == "drop_last_k":
        kcut = K - 1
    elif perturb == "drop_last_tile":
        kcut = (K - 1) // 64 * 64
    rows = []
    for r0, r1, slices in parts:
        if perturb == "drop_last_slice" and len(slices) > 1:
            slices = slices[:-1]
        total = torch.zeros(r1 - r0, n)
        for k0, k1 in slices:
            acc = torch.zeros(r1 - r0, n)
            for t0 in range(k0, min(k1, kcut), 64):
                t1 = min(t0 + 64, k1, kcut)
                acc = acc + Lf[r0:r1, t0:t1] @ Rf[t0:t1]
            total = total + acc
        if perturb == "dup_tail_row":
            # a tail token row clamped to the last valid one, not zero-filled
            total = total + Lf[r0:r1, K - 1:K] @ Rf[K - 1:K]
        rows.append(total)
    v = torch.cat(rows)
    assert v.dtype == torch.float32
    if bias is not None:
        b = bias.float()
        v = v + (torch.roll(b, 1) if perturb == "bias_shift" else b)
    if c["epi"] == 1 and perturb != "relu_missing":
        v = v.clamp(min=0)
    out = _bf16_trunc(v) if perturb == "truncate" else v.bfloat16()
    if perturb == "last_row_stale":
        out[-1] = STALE
    elif perturb == "last_col_stale":
        out[:, -1] = STALE
    elif perturb == "transpose_4x4":
        out[:4, :4] = out[:4, :4].t().clone()
    return out


def perturb_applies(name, perturb):
    c = case(name)
    if perturb == "drop_last_slice":
        return any(len(s) > 1 for _, _, s in emu_plan(c)[2])
    if perturb == "dup_tail_row":
        # only gemm_dw has a contraction tail that must be zero-filled
        return c["kernel"] == "gemm_dw" and c["K"] % 64 != 0
    if perturb == "bias_shift":
        return c["bias"]
    if perturb == "relu_missing":
        return c["epi"] == 1
    if perturb == "truncate":
        # the integer reference holds values that bf16 cannot (sums past
        # 256) and that round up
        L, R, bias, ref = emu_inputs(name, "int")
        v = ref[0].clamp(min=0) if c["epi"] == 1 else ref[0]
        v = v.float()
        return not torch.equal(_bf16_trunc(v).float(), v.bfloat16().float())
    return True


def accepts(name, kind, got):
    """Whether check (a) / (b) lets `got` through (emulation shapes)."""
    c = case(name)
    L, R, bias, ref = emu_inputs(name, kind)
    try:
        check(kind, got, L, R, bias, c["epi"], f"{name} {kind}", ref)
    except AssertionError:
        return False
    return True
