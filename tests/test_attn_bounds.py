"""The limits of tests/test_gpu_attn_elementwise.py, checked without a GPU.

Admit: for every case an fp32 torch emulation of the attention kernels (their
order of operations and their bf16 roundings, tests/_attn_cases.py) must pass
the SAME five checks against the fp64 reference that the HIP kernels face: a
limit that correct fp32 arithmetic cannot meet fails here.

Bite: the emulation made wrong the way a subtly wrong kernel would be (one
key too many or too few per row, a stale lse, D of the wrong row, a missing
scale) must fail at least one of the checks named for that mistake, on every
case the mistake applies to.

Identity: the fp64 reference is reference.scaled_dot_product_attention in
fp64 with the project's masks, on the rows that see a key."""

import pytest
import torch

import _attn_cases as C

# the outputs at least one of which must reject each perturbation
BITES = {
    "causal_plus_1": ("O", "LSE", "dQ", "dK", "dV"),
    "drop_last_live": ("O", "LSE", "dK", "dV"),
    "pad_key_live": ("O", "LSE", "dK", "dV"),
    "tail_key_live": ("O", "LSE"),
    "lse_stale": ("dQ", "dK", "dV"),
    "D_from_unrounded_O_wrong_row": ("dQ", "dK"),
    "scale_missing": ("dQ",),
}

BITE_PARAMS = [(p, n) for p in C.PERTURBS for n in C.CASES
               if C.perturb_applies(n, p)]


@pytest.mark.parametrize("name", C.CASES)
def test_attn_bounds_admit_fp32(name):
    c = C.attn_case(name)
    outs = C.attn_emulate(name)
    which = C.OUTPUTS if c["bwd"] else ("O", "LSE")
    C.check_all(name, outs, f"emu {name}", which)


def test_every_perturbation_has_cases():
    for p in C.PERTURBS:
        assert sum(q == p for q, _ in BITE_PARAMS) >= 5, p
    assert set(BITES) == set(C.PERTURBS)


@pytest.mark.parametrize("perturb,name", BITE_PARAMS)
def test_attn_checks_bite(perturb, name):
    outs = C.attn_emulate(name, perturb)
    raised = []
    for w in BITES[perturb]:
        try:
            C.check_output(name, w, outs[w], f"{perturb} {name}")
        except AssertionError as e:
            assert "err/limit" in str(e), e
            raised.append(w)
    print(f"{perturb} {name}: rejected by {raised}")
    assert raised, f"{perturb} on {name}: no check of {BITES[perturb]} bites"


def test_zero_demands_bite():
    """A value inside every limit's size, but where exact zeros are
    demanded: dV at a padded key, O at an id-0 row of the segment kernels."""
    name = "self-S65-dh64-c0-pad5"
    outs = C.attn_emulate(name)
    dv = outs["dV"].clone()
    dv[0, 62, 1, 3] = 1e-30
    with pytest.raises(AssertionError, match="err/limit"):
        C.check_output(name, "dV", dv)
    name = "seg-self-dh64-c0"
    outs = C.attn_emulate(name)
    o = outs["O"].clone()
    assert not bool(C.attn_case(name)["inc"][0, 190])
    o[0, 190, 1, 3] = 1e-30
    with pytest.raises(AssertionError, match="rows without a key"):
        C.check_output(name, "O", o)
    o = outs["O"].clone()
    o[2, 5, 0, 0] = float("inf")
    with pytest.raises(AssertionError, match="non-finite"):
        C.check_output(name, "O", o)


@pytest.mark.parametrize("name", C.IDENTITY_CASES)
def test_reference_is_the_projects_attention(name):
    import transformer_amd.ops.reference as R
    c, r = C.attn_case(name), C.attn_ref(name)
    q, k, v = (c[n].double().permute(0, 2, 1, 3).requires_grad_(True)
               for n in ("q", "k", "v"))
    if c["q_seg"] is not None:
        mask = R.create_segment_mask(c["q_seg"], c["kv_seg"], c["causal"])
    else:
        mask = c["kv_pad"].double()[:, None, None, :]
        if c["causal"]:
            la = R.create_look_ahead_mask(c["Sq"])
            mask = torch.maximum(mask, la[None, None].double())
    out = R.scaled_dot_product_attention(q, k, v, mask.double())
    assert out.dtype == torch.float64
    out.backward(c["do"].double().permute(0, 2, 1, 3))
    inc = c["inc"]
    assert int(inc.sum()) > 0
    for w, t in (("O", out.detach()), ("dQ", q.grad), ("dK", k.grad),
                 ("dV", v.grad)):
        t, ref = t.permute(0, 2, 1, 3), r[w]
        if w in ("O", "dQ"):
            t, ref = t[inc], ref[inc]
        err = float((t - ref).abs().max())
        print(f"{name} {w}: max |diff| = {err:.3e}")
        assert err <= 1e-12, (name, w, err)
