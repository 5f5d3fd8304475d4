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
