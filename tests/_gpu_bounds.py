"""Element-wise bounds shared by the GPU tests.

u = 2^-8 is the bf16 unit roundoff: a bf16 result of an fp32 sum is within
u*|ref| of the exact value, plus 1e-5 * sum|terms| for the fp32 summation
order.  Two such results (the same sum taken in two orders, each rounded to
bf16) are each inside that bound, so they are compared at twice it."""

import contextlib
import os

import torch

U = 2.0 ** -8


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _check(got, ref, absterm, name):
    """|got - ref| <= u*|ref| + 1e-5*absterm, element-wise."""
    got, ref = got.float(), ref.float()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    err = (got - ref).abs()
    lim = U * ref.abs() + 1e-5 * absterm
    worst = float((err / lim.clamp(min=1e-30)).max())
    print(f"{name}: max err/limit = {worst:.4f}")
    assert bool((err <= lim).all()), f"{name}: max err/limit {worst:.3f}"


def _check_pair(a, b, name):
    """Two bf16 roundings of one sum taken in two orders (see module doc);
    sum|terms| >= |sum|, so |b| stands in for it (stricter)."""
    a, b = a.float(), b.float()
    m = torch.maximum(a.abs(), b.abs())
    err = (a - b).abs()
    lim = 2 * U * m + 2e-5 * m
    worst = float((err / lim.clamp(min=1e-30)).max())
    print(f"{name}: max pair err/limit = {worst:.4f}")
    assert bool((err <= lim).all()), f"{name}: pair err/limit {worst:.3f}"


def _check_lim(got, ref, lim, name):
    """|got - ref| <= lim element-wise, in fp64 (nothing is rounded on the
    way to the comparison); prints the worst err/limit like _check."""
    got, ref, lim = got.double(), ref.double(), lim.double()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    assert bool(torch.isfinite(got).all()), f"{name}: non-finite output"
    err = (got - ref).abs()
    ratio = torch.where(err > 0, err / lim, torch.zeros_like(err))  # 0/0 -> 0
    worst = float(ratio.max()) if err.numel() else 0.0
    print(f"{name}: max err/limit = {worst:.4f}")
    assert bool((err <= lim).all()), f"{name}: max err/limit {worst:.3f}"


def _check_u(got, ref, absterm, name, u=U, extra=0.0):
    """_check's form against an fp64 reference:
    u*|ref| + 1e-5*absterm (+ extra, a term the caller derives)."""
    ref = ref.double()
    _check_lim(got, ref, u * ref.abs() + 1e-5 * absterm + extra, name)


def _check_f32(got, ref, absterm, name):
    """fp32 outputs carry no bf16 rounding: |got - ref| <= 1e-5*absterm."""
    _check_u(got, ref, absterm, name, u=0.0)


# ---------------------------------------------------------------------------
# numpy oracle of the dropout stream (dropout.hip pcg_hash, layernorm.hip
# ln_pcg): uint64 arithmetic that wraps, as the device's does.
# ---------------------------------------------------------------------------

_M64 = (1 << 64) - 1


def pcg_hash(key):
    """uint64 array -> uint32 array."""
    import numpy as np
    with np.errstate(over="ignore"):
        key = key.astype(np.uint64) * np.uint64(6364136223846793005) \
            + np.uint64(1442695040888963407)
        x = ((key ^ (key >> np.uint64(33))) >> np.uint64(11)) \
            .astype(np.uint32)
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7feb352d)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846ca68b)
        x ^= x >> np.uint32(16)
    return x


def dropout_threshold(p):
    import numpy as np
    return np.uint32(np.float32(p) * np.float32(4294967296.0))


def dropout_inv_keep(p):
    """The fp32 1/(1-p) the host passes to the kernels, as a Python float."""
    import numpy as np
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def dropout_keep(n, p, seed, counter=None):
    """Keep mask (uint8 numpy, 1 = kept) of elements 0..n-1: element i is
    kept iff pcg_hash(seed*0x9E3779B97F4A7C15 + i) >= threshold.  With the
    device counter (the seed_t argument) the seed is first replaced by
    seed*0xD1342543DE82EF95 + counter."""
    import numpy as np
    seed = int(seed) & _M64
    if counter is not None:
        seed = (seed * 0xD1342543DE82EF95 + int(counter)) & _M64
    base = (seed * 0x9E3779B97F4A7C15) & _M64
    with np.errstate(over="ignore"):
        key = np.uint64(base) + np.arange(n, dtype=np.uint64)
    return (pcg_hash(key) >= dropout_threshold(p)).astype(np.uint8)
