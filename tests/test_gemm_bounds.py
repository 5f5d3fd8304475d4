"""The checks of tests/test_gpu_gemm_elementwise.py proven on the CPU.

dispatch: the host arithmetic replayed in _gemm_cases (gemm_launch's sk /
k_per_slice, gemm_dw's nslices / m_per_slice, gemm_uni_launch's BN / nslices,
gemm256_tile, _dw_gemm's branch) puts every case on the arm its table row
names, and the arms that no earlier test reached are all reached.

admit: an fp32 emulation of the kernels (64-deep K tiles summed one after
another, fp32 slice sums, bias, ReLU, one bf16 rounding) passes check (a) and
check (b) on every element of every case.

bite: each subtly wrong variant of the emulation is rejected by (a) or (b) on
every case it applies to, and by the exact check (b) on at least one.

The cases with an output extent past 1024 are emulated at 256 + their ragged
remainder (the emulation has no tiles along M and N); the dispatch test holds
the full shapes.
"""

import pytest
import torch

import _gemm_cases as G


@pytest.mark.parametrize("name", G.CASES)
def test_dispatch_arm(name):
    c = G.case(name)
    p = G.plan(c)
    assert p["arm"] == c["arm"], (name, p["arm"])
    # the slices cover the contraction once, in order
    for r0, r1, slices in p["parts"]:
        assert slices[0][0] == 0 and slices[-1][1] == c["K"]
        assert all(a[1] == b[0] for a, b in zip(slices, slices[1:]))
    assert p["parts"][0][0] == 0 and p["parts"][-1][1] == c["M"]
    # the emulation's slices are the full shape's
    m, n, parts = G.emu_plan(c)
    assert [s for _, _, s in parts] == [s for _, _, s in p["parts"]]
    if c["kernel"].startswith("uni"):
        assert c["K"] % 64 == 0 and c["K"] >= 128


@pytest.mark.parametrize("label", list(G.REACHED))
def test_every_named_instantiation_is_reached(label):
    hit = [n for n in G.CASES if G.REACHED[label](G.case(n))]
    print(label, "<-", hit)
    assert hit, label


def test_named_slice_layouts():
    """The slice layouts the issue spells out."""
    P = lambda n: G.plan(G.case(n))["parts"][0][2]
    assert P("gemm128_nt-129x65x321-bias-epi1") == \
        [(0, 128), (128, 256), (256, 321)]
    assert P("gemm_dw-130x70x200")[-1] == (192, 200)        # tail of 8
    assert len(P("gemm_dw-128x128x4160")) == 65
    s = P("gemm_dw-641x641x1000")
    assert len(s) == 8 and s[-1] == (896, 1000)             # 64 + 40 rows
    assert P("uni_tn-300x200x192-s2") == [(0, 128), (128, 192)]
    assert P("uni_tn-300x200x192-s64") == [(0, 64), (64, 128), (128, 192)]
    parts = G.plan(G.case("dw_gemm-8194x128x192"))["parts"]
    assert [(a, b) for a, b, _ in parts] == [(0, 8192), (8192, 8194)]
    assert [len(s) for _, _, s in parts] == [1, 3]
    # old test_gemm_dw comment: (200,130,70) is four slices, not one
    assert G.gemm_dw_plan(200, 130, 70)["nslices"] == 4


def test_limit_constants():
    assert not G.C_TRUNC
    assert G.c_of(24) == 1e-5 and G.c_of(1024) == 1026 * 2.0 ** -24
    assert G.U == 2.0 ** -8


@pytest.mark.parametrize("kind", ["rand", "int"])
@pytest.mark.parametrize("name", G.CASES)
def test_admit(name, kind):
    got = G.emulate(name, kind)
    c = G.case(name)
    L, R, bias, ref = G.emu_inputs(name, kind)
    assert got.dtype == torch.bfloat16
    G.check(kind, got, L, R, bias, c["epi"], f"emu {name} {kind}", ref)
    if c["db"]:
        G.check_db(kind, L.float().sum(1).bfloat16(), L, f"emu {name} {kind}")


@pytest.mark.parametrize("perturb", G.PERTURBS)
def test_bite(perturb):
    applied, by_exact = [], []
    for name in G.CASES:
        if not G.perturb_applies(name, perturb):
            continue
        applied.append(name)
        rej_int = not G.accepts(name, "int", G.emulate(name, "int", perturb))
        rej = rej_int or not G.accepts(name, "rand",
                                       G.emulate(name, "rand", perturb))
        assert rej, f"{perturb} passes both checks on {name}"
        if rej_int:
            by_exact.append(name)
    print(f"{perturb}: {len(applied)} cases, {len(by_exact)} by the exact "
          f"check")
    assert applied, perturb
    assert by_exact, f"{perturb}: the exact check rejects it nowhere"
    if perturb == "truncate":
        # rounding has to happen for this one: integer sums past 256, and
        # the exact check is the one that tells
        assert by_exact == applied


def test_perturbations_apply_widely():
    """No perturbation is proven on a corner only."""
    n = {p: sum(G.perturb_applies(c, p) for c in G.CASES) for p in G.PERTURBS}
    print(n)
    assert n["drop_last_k"] == len(G.CASES)
    assert n["drop_last_slice"] >= 15 and n["dup_tail_row"] >= 8
    assert n["bias_shift"] >= 20 and n["relu_missing"] >= 10
    assert n["truncate"] >= 8
