"""dm_ssd_fwd at the wide states (d_state 32, 64, 128; csrc/ssd.hip, ssd_fwd_wide_kernel): the parts that need no GPU.

The reference, the four head regimes, the emulation and the forward bound are those of tests/test_ssd_gpu.py (read its docstring
first); what is restated here takes the state width N (and the head count) as an argument where that file has a module constant:
the input builder, `_seq`, and the forward half of `_bounds`.  The only constant of the bound that changes is the term count of the
state sum, an fp32 accumulation over N instead of 16 products:
    K0 = 72 + 2 (N - 16) + 2 (l + 1)
Everything else is charged as there: at most three 16-bit roundings per (query, key) pair before the second product (the B rows,
the C rows, the score tile) and one in the epilogue.  The wide kernel spends fewer (its B and C rows stay as given, gamma dt and
alpha delta multiply the fp32 accumulator), which the bound allows; the emulation `_manual` rounds at all three places.

Three defects are added that only a loop over 16-state slices can have, each applied to B in the fp64 reference:
    last16_dropped   the last 16 states zeroed (the loop stops one slice early)
    first16_only     every state from the 17th on zeroed (the d_state 16 contraction at a wide state)
    slices_crossed   the first two 16-state slices exchanged (B's slice k against C's slice k ^ 1)
They must exceed 4 x the bound at every L >= 31; at L = 1 the single score is one product per state and two of them stay below 4 at
N = 128 in bf16, so L = 1 is not named for them.

More heads than four (the head-count test of tests/test_ssd_wide_gpu.py) cycle the four regimes.
"""
import functools

import pytest
import torch

from tests.test_ssd_gpu import (A_H, BF16, BIAS_H, D_H, DEFECTS, DT_LEVEL, EPS32, F16, FWD_L, NAME, P, TILE, TINY, UNIT,
                                _decay, _dual, _manual, _ratio, _silu, _softplus)

WIDTHS = [32, 64, 128]
LS = sorted(FWD_L)
OUT_DEFECTS = {k: v[1] for k, v in DEFECTS.items() if v[0] == "out"}                     # drop_far, delta_prev, diag_mask, prev_head_A, table0
# Added to the seed of test_ssd_gpu.py's builder (1000 L + dtype) per width.  0 gives, draw for draw, that builder's stream at width
# N.  At N = 32 that stream leaves ONE named defect below 4 x its bound (delta_prev, bf16, L = 223, a single sequence: 2.05 -- the far
# pairs of that draw weigh at most 3.8 bounds on the mid and ends heads even when dropped altogether), so the GPU test could not tell
# that defect from the reference on those inputs.  2 is the smallest even salt (odd ones are the other dtype's seeds) at which every
# named defect exceeds 4 x at N = 32 in both dtypes (worst 4.77).  The choice looks only at the fp64 reference, the defects and the
# bound, never at a kernel's output; the bound, the 4 x, the cases and the lengths are untouched.
SEED_SALT = {32: 2, 64: 0, 128: 0}
SLICE_DEFECTS = {k: [L for L in LS if L >= 31] for k in ("last16_dropped", "first16_only", "slices_crossed")}


def head_params(nh):
    """A, D, dt_bias [nh]: the four regimes of test_ssd_gpu.py, cycled."""
    reg = torch.arange(nh) % 4
    return A_H[reg], D_H[reg], BIAS_H[reg]


@functools.lru_cache(maxsize=None)
def inputs(L, dtype, N, nh=4):
    """Host tensors of one case, as test_ssd_gpu._inputs with the state width and the head count as arguments."""
    ndir, bpd = FWD_L[L]
    S, din = ndir * bpd, nh * P
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    reg = torch.arange(nh) % 4
    spike = (torch.arange(L)[None] + 7 * torch.arange(bpd)[:, None]) % 40 == 5
    if nh == 4:                                                                          # draw for draw the builder of test_ssd_gpu.py
        g = torch.Generator().manual_seed(1000 * L + SEED_SALT[N] + (1 if dtype == F16 else 0))
        xBC, z, dout = rn(S, L, din + 2 * N).to(dtype), rn(bpd, L, din).to(dtype), rn(S, L, din).to(dtype)
        pre = torch.log(torch.expm1(DT_LEVEL * torch.exp(0.3 * rn(bpd, L, 3))))
        ends = -12.0 + 0.3 * rn(bpd, L)
        ends = torch.where(spike, (25.0 * torch.exp(0.3 * rn(bpd, L))).clamp_min(20.5), ends)
        raw = torch.cat([pre, ends[..., None]], -1)
    else:                                                                                # the same regimes, cycled over the heads
        g = torch.Generator().manual_seed(1000 * L + 10 * nh + (1 if dtype == F16 else 0))
        xBC, z, dout = rn(S, L, din + 2 * N).to(dtype), rn(bpd, L, din).to(dtype), rn(S, L, din).to(dtype)
        pre = torch.log(torch.expm1(DT_LEVEL[reg.clamp_max(2)] * torch.exp(0.3 * rn(bpd, L, nh))))
        ends = -12.0 + 0.3 * rn(bpd, L, nh)
        ends = torch.where(spike[..., None], (25.0 * torch.exp(0.3 * rn(bpd, L, nh))).clamp_min(20.5), ends)
        raw = torch.where(reg == 3, ends, pre)
    dt_tok = (raw - BIAS_H[reg]).to(dtype)                                               # (dout: _manual wants one; the forward ignores it)
    zperm = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)])
    operm = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)])
    return dict(L=L, dtype=dtype, N=N, nh=nh, ndir=ndir, bpd=bpd, S=S, xBC=xBC, z=z, dout=dout, dt_tok=dt_tok, zperm=zperm, operm=operm)


def seq(c, s, table0=False):
    """fp64 operands of sequence s in scan order, as test_ssd_gpu._seq."""
    k, b = divmod(s, c["bpd"])
    zi, oi = c["zperm"][0 if table0 else k], c["operm"][0 if table0 else k]
    L, N, nh = c["L"], c["N"], c["nh"]
    din = nh * P
    d = lambda t: t.double()
    return dict(x=d(c["xBC"][s, :, :din]).view(L, nh, P), B=d(c["xBC"][s, :, din:din + N]), C=d(c["xBC"][s, :, din + N:]),
                pre=d(c["dt_tok"][b])[zi] + head_params(nh)[2], z=d(c["z"][b])[zi].view(L, nh, P), dout=d(c["dout"][s])[oi].view(L, nh, P),
                zi=zi, oi=oi)


@functools.lru_cache(maxsize=None)
def unit_gate():
    """z0 with silu(z0) = 1 (1.27846...): the fp64 functions multiply by silu(z), and with this gate that factor is the identity to
    an ulp of fp64 -- the operator without a gate, out = Y + D x."""
    z0 = torch.tensor(1.0, dtype=torch.float64)
    for _ in range(60):                                                                  # Newton on z sigmoid(z) = 1
        sg = torch.sigmoid(z0)
        z0 = z0 - (z0 * sg - 1.0) / (sg * (1.0 + z0 * (1.0 - sg)))
    return float(z0)


def fwd_bound(q, A, D, dtype, ref_out, gate=True):
    """The forward bound of test_ssd_gpu.py's docstring for one sequence (scan order), K0 = 72 + 2 (N - 16) + 2 (l + 1).  gate False:
    the operator without a gate -- the factor silu(z) is 1 and its fp32 error term c_z is not charged."""
    u, T = UNIT[dtype], TINY[dtype]
    L, N = q["B"].shape
    nh = A.shape[0]
    x, Bm, Cm, z, pre = q["x"].abs(), q["B"].abs(), q["C"].abs(), q["z"], q["pre"]
    dt = _softplus(pre)
    s = A * dt.cumsum(0)
    sT, dtT = s.t(), dt.t()
    idx = torch.arange(L)
    tl = idx // TILE
    causal = (idx[:, None] >= idx[None, :])[None]
    M = _decay(s, L)
    Mdt = M * dtT[:, None, :]
    middle = (pre <= 20.0) & (torch.exp(pre) >= 2.0 ** -12)
    eps_dt = EPS32 * (torch.where(middle, 2.0 / dt, torch.zeros_like(dt)) + 2 * pre.abs() + 10)
    errs = (A.abs() * (eps_dt * dt).cumsum(0)).t()
    C32 = EPS32 * 12 * (sT.abs()[:, :, None] + sT.abs()[:, None, :]) + (errs[:, :, None] - errs[:, None, :]).clamp_min(0) + eps_dt.t()[:, None, :]
    Wabs = (Cm @ Bm.t())[None] * Mdt
    cz = EPS32 * (2 * z.abs() + 12) if gate else torch.zeros_like(z)
    silu = _silu(z).abs() if gate else torch.ones_like(z)
    mm = lambda E, v: torch.einsum("hli,ihp->lhp", E, v)
    m = torch.cat([torch.zeros(nh, 1, dtype=s.dtype), sT[:, TILE - 1::TILE], sT[:, -1:]], 1)
    alpha, gamma = torch.exp(sT - m[:, tl]), torch.exp(m[:, tl + 1] - sT)
    delta = torch.exp((m[:, tl][:, :, None] - m[:, tl + 1][:, None, :]).clamp_max(0))
    off = (tl[:, None] > tl[None, :])[None]
    P1 = torch.where(off, delta * (gamma * dtT)[:, None, :], Mdt)
    P2 = torch.where(off, delta * alpha[:, :, None], M)
    K0f = EPS32 * (72 + 2 * (N - 16) + 2 * (idx + 1.0))[None, :, None]
    Ef = ((1 + u) ** 3 - 1 + C32 + K0f) * Wabs + T * ((1 + u) ** 2 * (P1 * Bm.sum(1)[None, None, :] + P2 * Cm.sum(1)[None, :, None]) + 1 + 17 * T) * causal
    Dx = D.abs()[None, :, None] * x
    return silu * mm(Ef, x) * (1 + u) * (1 + cz) + 4 * EPS32 * silu * (mm(Wabs, x) + Dx) + (u + cz) * ref_out.abs() + T


def _rows(v, oi, L):
    return torch.empty_like(v).index_copy_(0, oi, v).reshape(L, -1)                     # step l lands in row out_row_index[l]


@functools.lru_cache(maxsize=None)
def analysis(L, dtype, N, nh=4, gate=True):
    """(ref, tol) [S, L, nh * P] of one case in the kernel's output layout: fp64 dual form and its bound.  Computed once per case.
    gate False: the same operands without the gate, out = Y + D x."""
    c = inputs(L, dtype, N, nh)
    A, D, _ = head_params(nh)
    ref, tol = [], []
    for s in range(c["S"]):
        q = seq(c, s)
        if not gate:
            q = {**q, "z": torch.full_like(q["z"], unit_gate())}
        out = _dual(q, A, D)
        ref.append(_rows(out, q["oi"], L))
        tol.append(_rows(fwd_bound(q, A, D, dtype, out, gate), q["oi"], L))
    return torch.stack(ref), torch.stack(tol)


def _emulation(L, dtype, N):
    """`out` of test_ssd_gpu._manual rounded at the three places and in the epilogue, and before that last rounding."""
    c = inputs(L, dtype, N)
    rnd = lambda v: v.to(dtype).double()
    out, pre = [], []
    for s in range(c["S"]):
        q = seq(c, s)
        e = _manual(q, A_H, D_H, rnd)
        out.append(_rows(e["out"], q["oi"], L))
        pre.append(_rows(e["out_pre"], q["oi"], L))
    return torch.stack(out), torch.stack(pre)


def _slice_defect(B, defect):
    B = B.clone()
    if defect == "last16_dropped":
        B[:, -16:] = 0
    elif defect == "first16_only":
        B[:, 16:] = 0
    elif defect == "slices_crossed":
        B[:, :32] = torch.cat([B[:, 16:32], B[:, :16]], 1)
    return B


def _defective(L, dtype, N, defect):
    c = inputs(L, dtype, N)
    res = []
    for s in range(c["S"]):
        q = seq(c, s, table0=(defect == "table0"))
        if defect in SLICE_DEFECTS:
            o = _dual({**q, "B": _slice_defect(q["B"], defect)}, A_H, D_H)
        else:
            o = _dual(q, A_H, D_H, defect=defect)
        res.append(_rows(o, q["oi"], L))
    return torch.stack(res)


# =====================================================================================================================================
def test_supported_set_names_the_wide_states():
    """The C ABI's answer per width: the forward takes d_state 16, 32, 64, 128 in both 16-bit dtypes up to L = 224, the backward
    stays at d_state 16, and the ABI version says so."""
    from diffma_amd import _lib

    lib = _lib.load()
    bf16, f16, f32 = _lib.DM_BF16, _lib.DM_F16, _lib.DM_F32
    for code in (bf16, f16):
        for L in (1, 196, 224):
            for N in (16, 32, 64, 128):
                assert lib.dm_ssd_fwd_supported(L, 64, N, code) == 1, (L, N, code)
            for N in (8, 24, 48, 256):
                assert lib.dm_ssd_fwd_supported(L, 64, N, code) == 0, (L, N, code)
        for N in (16, 32, 64, 128):
            assert lib.dm_ssd_fwd_supported(225, 64, N, code) == 0
            assert lib.dm_ssd_fwd_supported(196, 32, N, code) == 0
    for N in (16, 32, 64, 128):
        assert lib.dm_ssd_fwd_supported(196, 64, N, f32) == 0
    for N in (32, 64, 128):
        assert lib.dm_ssd_bwd_supported(196, 64, N, bf16) == 0
    assert lib.dm_ssd_bwd_supported(196, 64, 16, bf16) == 1
    assert lib.dm_abi_version() >= 31 and _lib.CONSTANTS["DM_ABI_VERSION"] >= 31


def test_routed_widths_are_served_widths():
    """hip_ops.SSD_FWD_WIDTHS: what the dispatch routes is a subset of what the C ABI serves, and holds Mamba-2's default."""
    from diffma_amd import _lib, hip_ops

    lib = _lib.load()
    assert {16, 64, 128} <= set(hip_ops.SSD_FWD_WIDTHS)
    assert all(lib.dm_ssd_fwd_supported(196, 64, N, _lib.DM_BF16) == 1 for N in hip_ops.SSD_FWD_WIDTHS)


@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_wide_bound_holds_for_the_emulation_with_margin(dtype, N):
    """The forward bound at width N against the emulation with all three roundings: <= 0.5 for `out` before its last rounding,
    <= 1 after it (one rounding that the bound charges in full), at every listed L."""
    worst = {"out": 0.0, "out_pre": 0.0}
    for L in LS:
        ref, tol = analysis(L, dtype, N)
        out, pre = _emulation(L, dtype, N)
        r, rp = float(_ratio(out, ref, tol).max()), float(_ratio(pre, ref, tol).max())
        worst = {"out": max(worst["out"], r), "out_pre": max(worst["out_pre"], rp)}
        assert rp <= 0.5 and r <= 1.0, (L, N, NAME[dtype], rp, r)
    print(N, NAME[dtype], {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("defect", list(OUT_DEFECTS) + list(SLICE_DEFECTS))
@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_wide_bound_tells_each_defect_from_the_reference(dtype, N, defect):
    """Each defect, applied to the fp64 reference, leaves at least one element more than 4 x its bound away at every L named for it.

    Figures on these inputs (worst ratio over the named L and both dtypes): the three slice defects >= 10.6 (last16_dropped, N = 128,
    bf16); N = 64 and 128: delta_prev >= 5.2, drop_far >= 5.5, diag_mask >= 9.6; N = 32 (SEED_SALT): every defect >= 4.77 (diag_mask,
    L = 1, fp16)."""
    seen = {}
    for L in {**OUT_DEFECTS, **SLICE_DEFECTS}[defect]:
        ref, tol = analysis(L, dtype, N)
        seen[L] = float(_ratio(_defective(L, dtype, N, defect), ref, tol).max())
    print(defect, N, NAME[dtype], {L: round(v, 1) for L, v in seen.items()})
    assert all(v > 4.0 for v in seen.values()), (defect, N, NAME[dtype], seen)
