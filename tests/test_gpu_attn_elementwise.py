"""The training attention kernels against an fp64 reference, element-wise.

attn_fwd / attn_bwd (modes 0/1/2) and attn_fwd_seg / attn_bwd_seg are called
on the extension itself, in the real chain: the backward gets the kernel's
own o and lse.  Cases, reference and limits are tests/_attn_cases.py; the
same checks are proven on an fp32 emulation in tests/test_attn_bounds.py.

Reached here: dh 32/64/128, both trv values, modes 0/1/2, the 32- and 64-row
backward tiles in the plain and the SEG instantiations, the forward's
explicit batch stride (cache slices) and a leading all-pad key tile."""

import pytest
import torch

import _attn_cases as C

pytestmark = pytest.mark.gpu


def _ext():
    from transformer_amd.ops import ext
    return ext()


def _contig(t, shape, dtype, tag):
    assert tuple(t.shape) == tuple(shape), (tag, tuple(t.shape))
    assert t.dtype == dtype and t.is_contiguous(), (tag, t.dtype, t.stride())


def _inputs(c):
    """Device q, k, v in the case's layout, dO, and the mask arguments."""
    B, Sq, Sk, H, dh = c["B"], c["Sq"], c["Sk"], c["H"], c["dh"]
    q, k, v = (c[n].cuda() for n in ("q", "k", "v"))
    if c["layout"] == "qkv":        # unbind(2) views of one (B,S,3,H,dh)
        q, k, v = torch.stack([q, k, v], dim=2).unbind(2)
        assert q.stride(1) == 3 * H * dh and not q.is_contiguous()
    elif c["layout"] == "kv":       # k/v views of one (B,Sk,2,H,dh)
        k, v = torch.stack([k, v], dim=2).unbind(2)
        assert k.stride(1) == 2 * H * dh
    elif c["layout"] == "cache":    # [:, :Sk] of a longer buffer, NaN behind
        kb, vb = (torch.full((B, Sk + 19, H, dh), float("nan"),
                             device="cuda", dtype=torch.bfloat16)
                  for _ in range(2))
        kb[:, :Sk], vb[:, :Sk] = k, v
        k, v = kb[:, :Sk], vb[:, :Sk]
        assert k.stride(0) != Sk * k.stride(1)
    pad = c["kv_pad"].cuda() if bool(c["kv_pad"].any()) else torch.Tensor()
    seg = None
    if c["q_seg"] is not None:
        seg = (c["q_seg"].cuda(), c["kv_seg"].cuda())
    return q, k, v, c["do"].cuda(), pad, seg


def _forward(c, q, k, v, pad, seg, trv):
    E = _ext()
    if seg is not None:
        o, lse = E.attn_fwd_seg(q, k, v, seg[0], seg[1], c["causal"],
                                c["scale"])
    else:
        o, lse = E.attn_fwd(q, k, v, pad, c["causal"], c["scale"], trv)
    B, Sq, H, dh = c["B"], c["Sq"], c["H"], c["dh"]
    _contig(o, (B, Sq, H, dh), torch.bfloat16, "o")
    _contig(lse, (B, H, Sq), torch.float32, "lse")
    return o, lse


def _backward(c, q, k, v, o, do, lse, pad, seg):
    E = _ext()
    B, Sq, Sk, H, dh = c["B"], c["Sq"], c["Sk"], c["H"], c["dh"]
    mode = {"plain": 0, "qkv": 1, "kv": 2}[c["layout"]]
    if seg is not None:
        out = E.attn_bwd_seg(q, k, v, o, do, lse, seg[0], seg[1],
                             c["causal"], c["scale"], mode)
    else:
        out = E.attn_bwd(q, k, v, o, do, lse, pad, c["causal"], c["scale"],
                         mode)
    bf = torch.bfloat16
    if mode == 1:
        (dqkv,) = out
        _contig(dqkv, (B, Sq, 3, H, dh), bf, "dqkv")
        return dqkv.unbind(2)       # slot by slot
    if mode == 2:
        dq, dkv = out
        _contig(dq, (B, Sq, H, dh), bf, "dq")
        _contig(dkv, (B, Sk, 2, H, dh), bf, "dkv")
        return (dq,) + tuple(dkv.unbind(2))
    dq, dk, dv = out
    _contig(dq, (B, Sq, H, dh), bf, "dq")
    _contig(dk, (B, Sk, H, dh), bf, "dk")
    _contig(dv, (B, Sk, H, dh), bf, "dv")
    return dq, dk, dv


@pytest.mark.parametrize("name", C.CASES)
def test_attn_elementwise(name):
    c = C.attn_case(name)
    q, k, v, do, pad, seg = _inputs(c)
    o, lse = _forward(c, q, k, v, pad, seg, c["trv"])
    outs = dict(O=o.cpu(), LSE=lse.cpu())
    if c["bwd"]:
        dq, dk, dv = _backward(c, q, k, v, o, do, lse, pad, seg)
        outs.update(dQ=dq.cpu(), dK=dk.cpu(), dV=dv.cpu())
    C.check_all(name, outs, f"gpu {name}", tuple(outs))


@pytest.mark.parametrize("trv", [0, 1])
@pytest.mark.parametrize("name", C.TRV_CASES)
def test_attn_fwd_both_v_operand_paths(name, trv):
    """trv = 0 builds a transposed V image in LDS, trv = 1 reads the natural
    one with the transposing load: the same limits hold for both."""
    c = C.attn_case(name)
    assert c["q_seg"] is None
    q, k, v, do, pad, seg = _inputs(c)
    o, lse = _forward(c, q, k, v, pad, None, trv)
    C.check_all(name, dict(O=o.cpu(), LSE=lse.cpu()), f"gpu trv={trv} {name}",
                ("O", "LSE"))


def test_attn_fwd_is_deterministic():
    c = C.attn_case("self-S129-dh64-c1-pad5")
    q, k, v, do, pad, seg = _inputs(c)
    o1, l1 = _forward(c, q, k, v, pad, seg, 1)
    o2, l2 = _forward(c, q, k, v, pad, seg, 1)
    assert torch.equal(o1.view(torch.int16), o2.view(torch.int16))
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
