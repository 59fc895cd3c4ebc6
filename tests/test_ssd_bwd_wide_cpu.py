"""dm_ssd_bwd_wide (d_state 32, 64, 128; csrc/ssd_bwd_wide.hip): the parts that need no GPU.

The reference (fp64 `_dual` under autograd), the four head regimes, the closed-form emulation `_manual` and the backward bounds are
those of tests/test_ssd_gpu.py (read its docstring first).  What is restated here takes the state width N and the head count as
arguments where that file has a module constant: the input builder (the one of tests/test_ssd_wide_cpu.py draw for draw, with the
directions and batches of BWD_L, which has L = 129), the backward half of `_bounds`, and the backward half of `_manual` for head
counts other than four.  Three constants of the bound change, all for the state sum, an fp32 accumulation over N instead of 16
products; nothing is taken from a measured error:
    C32b:   256 + 4 L           ->  256 + 2 (N - 16) + 4 L
    E32V:   256 + L             ->  256 + 2 (N - 16) + L
    E32V:   32 Gabs |R|         ->  2 N Gabs |R|
The kernel rounds to 16 bits where ssd_bwd.hip does and nowhere else: the stored gY, the W tile, the dG tile, dz and dx on the way
out.  dB / dC leave in fp32; the two heads of a workgroup are added in fp32 before the partial rows leave it and the caller's column
sum adds the groups: H - 1 fp32 additions per element in all, as many as the d_state 16 kernel's sum over heads, so the flat
constant is not raised.

Defects, each applied to the fp64 reference, must exceed 4 x the bound on the cases named below: `no_A_term` (d dt), `dA_near` (dA),
and the slice defects `last16_dropped` / `slices_crossed` of tests/test_ssd_wide_cpu.py, applied to B and looked for in dx, dz, dC,
applied to C and looked for in dB.
"""
import functools
import os

import pytest
import torch

from tests.test_ssd_gpu import (A_H, BF16, BIAS_H, BWD_L, D_H, DT_LEVEL, EPS32, F16, GRADS, NAME, P, TINY, UNIT, _decay, _dual, _manual,
                                _ratio, _silu, _softplus)
from tests.test_ssd_wide_cpu import SEED_SALT, WIDTHS, _slice_defect, head_params, seq

LS = sorted(BWD_L)                                                                       # 1, 32, 33, 65, 97, 129, 196
NO_A_TERM_L = [L for L in LS if L >= 32]
DA_NEAR = {(F16, 32): [97, 129], (F16, 64): [97, 129], (F16, 128): [129], (BF16, 64): [129], (BF16, 128): [129]}   # bf16 at N 32: 2.5 at most
SLICE_L = [L for L in LS if L >= 32]                                                      # L = 1: N 128 in bf16 gives 1.3
SLICE_SEEN_IN = {"B": ["dx", "dz", "dC"], "C": ["dB"]}


@functools.lru_cache(maxsize=None)
def inputs(L, dtype, N, nh=4):
    """Host tensors of one case: the builder of tests.test_ssd_wide_cpu.inputs draw for draw, (directions, batch_per_dir) from BWD_L."""
    ndir, bpd = BWD_L[L]
    S, din = ndir * bpd, nh * P
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    reg = torch.arange(nh) % 4
    spike = (torch.arange(L)[None] + 7 * torch.arange(bpd)[:, None]) % 40 == 5
    if nh == 4:
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
    dt_tok = (raw - BIAS_H[reg]).to(dtype)
    zperm = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)])
    operm = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)])
    return dict(L=L, dtype=dtype, N=N, nh=nh, ndir=ndir, bpd=bpd, S=S, xBC=xBC, z=z, dout=dout, dt_tok=dt_tok, zperm=zperm, operm=operm)


def bwd_bound(q, A, D, dtype, ref):
    """The backward half of test_ssd_gpu._bounds for one sequence (scan order) with the state width and the head count read off the
    operands; the three constants of the module docstring carry N."""
    u, T = UNIT[dtype], TINY[dtype]
    L, N = q["B"].shape
    x, Bm, Cm, z, do, pre = q["x"].abs(), q["B"].abs(), q["C"].abs(), q["z"], q["dout"], q["pre"]
    xs = q["x"]
    dt = _softplus(pre)
    cum = dt.cumsum(0)
    s = A * cum
    sT, dtT = s.t(), dt.t()
    idx = torch.arange(L)
    causal = (idx[:, None] >= idx[None, :])[None]
    M = _decay(s, L)
    Mdt = M * dtT[:, None, :]
    middle = (pre <= 20.0) & (torch.exp(pre) >= 2.0 ** -12)
    eps_dt = EPS32 * (torch.where(middle, 2.0 / dt, torch.zeros_like(dt)) + 2 * pre.abs() + 10)
    errs = (A.abs() * (eps_dt * dt).cumsum(0)).t()
    C32 = EPS32 * 12 * (sT.abs()[:, :, None] + sT.abs()[:, None, :]) + (errs[:, :, None] - errs[:, None, :]).clamp_min(0) + eps_dt.t()[:, None, :]
    Gabs = (Cm @ Bm.t())[None]
    Wabs = Gabs * Mdt
    cz = EPS32 * (2 * z.abs() + 12)
    mm = lambda E, v: torch.einsum("hli,ihp->lhp", E, v)
    Dx = D.abs()[None, :, None] * x
    sg = torch.sigmoid(z)
    sig = torch.where(pre > 20.0, torch.ones_like(dt), torch.sigmoid(pre))
    gy = (do * _silu(z)).abs()
    dg = (u + cz) * gy + T
    C32b = C32 + EPS32 * (256 + 2 * (N - 16) + 4 * L)
    Rabs = torch.einsum("lhp,ihp->hli", gy, x) * causal
    dR = torch.einsum("lhp,ihp->hli", dg, x) * causal
    EW = (u + C32b) * Wabs + T * causal
    spabs = sg * (1 + z.abs() * (1 - sg))
    tol = {}
    tol["dz"] = do.abs() * spabs * (mm(EW, x) * (1 + u) + (cz + 4 * EPS32) * (mm(Wabs, x) + Dx)) + (u + cz) * ref["dz"].abs() + T
    tol["dx"] = (torch.einsum("hli,lhp->ihp", EW, gy * (1 + u) + T) + torch.einsum("hli,lhp->ihp", Wabs, dg) + D.abs()[None, :, None] * dg
                 + 4 * EPS32 * D.abs()[None, :, None] * gy) * (1 + u) + u * ref["dx"].abs() + T
    EdG = u * (Rabs + dR) * Mdt + dR * Mdt + C32b * Rabs * Mdt + T * causal
    tol["dB"] = torch.einsum("hli,ln->in", EdG, Cm)
    tol["dC"] = torch.einsum("hli,in->ln", EdG, Bm)
    Vabs = Rabs * Gabs * M
    Veps = dR * Gabs * M + C32b * Vabs
    csig = EPS32 * (2 * pre.abs() + 10).t()
    inner = lambda V: (V @ dtT[:, :, None]).squeeze(2) + dtT * V.sum(1)
    F = lambda V: sig.t() * (V.sum(1) + A.abs()[:, None] * inner(V).flip(1).cumsum(1).flip(1))
    tol["ddt"] = (F(Veps) + csig * F(Vabs)).t()
    Rs = torch.einsum("lhp,ihp->hli", do * _silu(z), xs) * causal
    Gs = (q["C"] @ q["B"].t())[None]
    E32V = M * (Rs.abs() * Gs.abs() * (C32 + EPS32 * (256 + 2 * (N - 16) + L)) + EPS32 * (2 * N * Gabs * Rs.abs() + 128 * Rabs * Gs.abs()))
    red = lambda Cf: (dg * torch.einsum("hli,ihp->lhp", Gs * M * Cf, xs).abs()).sum((0, 2))
    cumT, sigT = cum.t(), sig.t()
    csum = sigT.cumsum(1)
    tol["dA"] = red(dtT[:, None, :] * (cumT[:, :, None] - cumT[:, None, :])) + (inner(E32V) * cumT).sum(1)
    tol["dbias"] = (red(sigT[:, None, :] + A[:, None, None] * dtT[:, None, :] * (csum[:, :, None] - csum[:, None, :]))
                    + (F(E32V) + csig * F(Rs.abs() * Gs.abs() * M)).sum(1))
    tol["dD"] = EPS32 * (2 * float(z.abs().max()) + 12 + 74) * (gy * x).sum((0, 2))
    return tol


def manual_bwd(q, A, D, rnd):
    """The backward half of test_ssd_gpu._manual (which is written for four heads): every gradient of one sequence in closed form,
    rounded where ssd_bwd.hip rounds."""
    r = rnd if rnd is not None else (lambda v: v)
    L = q["x"].shape[0]
    x, Bm, Cm, z, do = q["x"], q["B"], q["C"], q["z"], q["dout"]
    dt = _softplus(q["pre"])
    sig = torch.where(q["pre"] > 20.0, torch.ones_like(dt), torch.sigmoid(q["pre"]))
    cum = dt.cumsum(0)
    M = _decay(A * cum, L)
    Mdt = M * dt.t()[:, None, :]
    G = (Cm @ Bm.t())[None]
    sg = torch.sigmoid(z)
    gy = do * _silu(z)
    gyr = r(gy)
    R = torch.einsum("lhp,ihp->hli", gyr, x)
    Wr = r(G * Mdt)
    dGr = r(R * Mdt)
    u_ = torch.einsum("hli,ihp->lhp", Wr, x) + D[None, :, None] * x
    dz_pre = do * u_ * sg * (1.0 + z * (1.0 - sg))
    dx_pre = torch.einsum("hli,lhp->ihp", Wr, gyr) + D[None, :, None] * gyr
    dB = torch.einsum("hli,ln->hin", dGr, Cm)                                            # per head
    dC = torch.einsum("hli,in->hln", dGr, Bm)
    V = R * G * M
    rs = (V * dt.t()[:, None, :]).sum(2)
    cs = V.sum(1)
    ds = rs - dt.t() * cs
    rc = ds.flip(1).cumsum(1).flip(1)
    draw = ((cs + A[:, None] * rc) * sig.t()).t()
    return dict(dx=r(dx_pre), dz=r(dz_pre), dx_pre=dx_pre, dz_pre=dz_pre, dB=dB.sum(0), dC=dC.sum(0), ddt=draw, dA=(ds * cum.t()).sum(1),
                dD=(gy * x).sum((0, 2)), dbias=draw.sum(0))


def _layout(k, v, q, L):
    """One sequence's tensor in the kernel's output layout: dz / d raw dt rows through z_row_index, dx / dB / dC in scan order."""
    if k in ("dz", "dz_pre", "ddt"):
        v = torch.empty_like(v).index_copy_(0, q["zi"], v)
    return v.reshape(L, -1) if v.dim() == 3 else v


def _stack(d):
    return {k: torch.stack(v).sum(0) if k in ("dA", "dD", "dbias") else torch.stack(v) for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def analysis(L, dtype, N, nh=4):
    """(ref, tol) of one case in the kernel's output layout: fp64 autograd through `_dual` and the bound.  Computed once per case."""
    c = inputs(L, dtype, N, nh)
    S = c["S"]
    A_, D_, _ = head_params(nh)
    A = A_.clone().requires_grad_(True)
    D = D_.clone().requires_grad_(True)
    shift = torch.zeros(nh, dtype=torch.float64, requires_grad=True)
    ref, tol = {}, {}
    for s in range(S):
        q = seq(c, s)
        leaves = {k: q[k].clone().requires_grad_(True) for k in ("x", "B", "C", "pre", "z")}
        out = _dual({**q, **leaves}, A, D, shift)
        ga, gd, gs = (None if t.grad is None else t.grad.clone() for t in (A, D, shift))
        (out * q["dout"]).sum().backward()
        part = lambda t, g0: t.grad.clone() if g0 is None else t.grad - g0
        r = dict(dx=leaves["x"].grad, dz=leaves["z"].grad, dB=leaves["B"].grad, dC=leaves["C"].grad, ddt=leaves["pre"].grad,
                 dA=part(A, ga), dD=part(D, gd), dbias=part(shift, gs))
        t = bwd_bound(q, A_, D_, dtype, r)
        for k in GRADS:
            ref.setdefault(k, []).append(_layout(k, r[k], q, L))
            tol.setdefault(k, []).append(_layout(k, t[k], q, L))
    ref, tol = _stack(ref), _stack(tol)
    for k in ("dA", "dD", "dbias"):                                                      # the sum over the sequences: S fp32 additions
        tol[k] = tol[k] * (1 + S * EPS32) + S * EPS32 * ref[k].abs()
    return ref, tol


def emulation(L, dtype, N, nh=4):
    """The closed form rounded at every place the kernel may round, in the layout of `analysis` (with dx_pre / dz_pre)."""
    c = inputs(L, dtype, N, nh)
    A_, D_, _ = head_params(nh)
    rnd = lambda v: v.to(dtype).double()
    emu = {}
    for s in range(c["S"]):
        q = seq(c, s)
        e = _manual(q, A_H, D_H, rnd) if nh == 4 else manual_bwd(q, A_, D_, rnd)
        for k in GRADS + ["dx_pre", "dz_pre"]:
            emu.setdefault(k, []).append(_layout(k, e[k], q, L))
    return _stack(emu)


def defective(L, dtype, N, defect, operand=None):
    """{output: tensor} of the fp64 closed form with one defect, in the layout of `analysis`."""
    c = inputs(L, dtype, N)
    res = {}
    for s in range(c["S"]):
        q = seq(c, s)
        if operand is None:
            m = _manual(q, A_H, D_H, None, defect)
        else:
            m = _manual({**q, operand: _slice_defect(q[operand], defect)}, A_H, D_H)
        for k in GRADS:
            res.setdefault(k, []).append(_layout(k, m[k], q, L))
    return _stack(res)


# =====================================================================================================================================
def test_wide_backward_entry_points_and_workspace():
    """dm_ssd_bwd_wide_supported is 1 exactly for 1 <= L <= 196, headdim 64, d_state 32 / 64 / 128, bf16 / f16 (0 at 16, which
    dm_ssd_bwd serves, whose own answer at the wide states stays 0); ABI 32; the partial rows of ceil(H / DM_SSD_BWD_WIDE_HEADS)
    groups never take more than the scan pair's dB / dC workspace (ceil(64 H / GC) rows per position, GC = 4096 / N)."""
    from diffma_amd import _lib

    lib = _lib.load()
    bf16, f16, f32 = _lib.DM_BF16, _lib.DM_F16, _lib.DM_F32
    for code in (bf16, f16):
        for N in WIDTHS:
            assert [lib.dm_ssd_bwd_wide_supported(L, 64, N, code) for L in (0, 1, 196, 197, 224)] == [0, 1, 1, 0, 0], (N, code)
            assert lib.dm_ssd_bwd_wide_supported(196, 32, N, code) == 0 and lib.dm_ssd_bwd_supported(196, 64, N, code) == 0
        for N in (8, 16, 24, 48, 256):
            assert lib.dm_ssd_bwd_wide_supported(196, 64, N, code) == 0, (N, code)
    assert all(lib.dm_ssd_bwd_wide_supported(196, 64, N, f32) == 0 for N in WIDTHS)
    assert lib.dm_abi_version() >= 32 and _lib.CONSTANTS["DM_ABI_VERSION"] >= 32
    HG = _lib.CONSTANTS["DM_SSD_BWD_WIDE_HEADS"]
    assert HG >= 1
    for N in WIDTHS:
        GC = 4096 // N
        for H in (2, 3, 8, 16, 24):
            assert -(-H // HG) <= -(-64 * H // GC), (N, H)


def test_routing_switch_is_off_by_default_and_routes_served_widths():
    """hip_ops.SSD_MFMA_BWD_WIDE follows DIFFMA_SSD_MFMA_BWD_WIDE (unset: off); what it routes is a subset of what the C ABI serves."""
    from diffma_amd import _lib, hip_ops

    assert hip_ops.SSD_MFMA_BWD_WIDE == (os.environ.get("DIFFMA_SSD_MFMA_BWD_WIDE", "0") == "1")
    lib = _lib.load()
    assert all(lib.dm_ssd_bwd_wide_supported(196, 64, N, _lib.DM_BF16) == 1 for N in hip_ops.SSD_BWD_WIDE_WIDTHS)
    assert 16 not in hip_ops.SSD_BWD_WIDE_WIDTHS


def test_restated_closed_form_is_the_module_one_at_four_heads():
    """manual_bwd (any head count) against test_ssd_gpu._manual (four heads), rounded, at N = 64, bf16, L = 65: the same numbers."""
    c = inputs(65, BF16, 64)
    rnd = lambda v: v.to(BF16).double()
    for s in range(c["S"]):
        q = seq(c, s)
        a, b = _manual(q, A_H, D_H, rnd), manual_bwd(q, A_H, D_H, rnd)
        for k in b:
            assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_wide_backward_bounds_hold_for_the_emulation_with_margin(dtype, N):
    """Every bound at width N against the emulation rounded at all listed places, every L of BWD_L: <= 0.5 for the fp32 outputs and
    for dx / dz before their last rounding, <= 1 for dx / dz after it (one rounding that the bound charges in full).  Worst figures
    on these inputs: fp32 outputs 0.374 (dC, N 64, bf16, L 196), dx_pre 0.495, dz_pre 0.483, dx 0.965, dz 0.985."""
    worst = {}
    for L in LS:
        ref, tol = analysis(L, dtype, N)
        emu = emulation(L, dtype, N)
        for k in emu:
            kr = k[:-4] if k.endswith("_pre") else k
            r = float(_ratio(emu[k], ref[kr], tol[kr]).max())
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= (1.0 if k in ("dx", "dz") else 0.5), (k, L, N, NAME[dtype], r)
    print(N, NAME[dtype], {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("nh", [2, 3, 16])
def test_wide_backward_bounds_hold_at_other_head_counts(nh):
    """The case of the GPU head-count test (N 128, bf16, L 65) with the regimes cycled over nh heads: the emulation against the bound
    restated with nh, same margins."""
    ref, tol = analysis(65, BF16, 128, nh)
    emu = emulation(65, BF16, 128, nh)
    for k in emu:
        kr = k[:-4] if k.endswith("_pre") else k
        r = float(_ratio(emu[k], ref[kr], tol[kr]).max())
        assert r <= (1.0 if k in ("dx", "dz") else 0.5), (k, nh, r)


@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_wide_backward_bounds_tell_the_dt_defects_from_the_reference(dtype, N):
    """no_A_term (d dt without A sum_{l >= i} d s_l) at every L >= 32 and dA_near (dA without the pairs two or more tiles apart) on
    the cases of DA_NEAR: more than 4 x the bound.  Smallest figures: no_A_term 4.3 (N 64, bf16, L 32); dA_near 6.1 (N 128, bf16, L 129)."""
    seen = {}
    for L in NO_A_TERM_L:
        ref, tol = analysis(L, dtype, N)
        seen[("no_A_term", L)] = float(_ratio(defective(L, dtype, N, "no_A_term")["ddt"], ref["ddt"], tol["ddt"]).max())
    for L in DA_NEAR.get((dtype, N), []):
        ref, tol = analysis(L, dtype, N)
        seen[("dA_near", L)] = float(_ratio(defective(L, dtype, N, "dA_near")["dA"], ref["dA"], tol["dA"]).max())
    print(N, NAME[dtype], {k: round(v, 1) for k, v in seen.items()})
    assert all(v > 4.0 for v in seen.values()), (N, NAME[dtype], seen)


@pytest.mark.parametrize("defect", ["last16_dropped", "slices_crossed"])
@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_wide_backward_bounds_tell_the_slice_defects_from_the_reference(dtype, N, defect):
    """A loop over 16-state slices that stops early or pairs the wrong slices: applied to B it must show in dx, dz and dC, applied to
    C in dB, by more than 4 x the bound at every L >= 32.  Smallest figures: last16_dropped 16.0 (dx), slices_crossed 31.4 (dx)."""
    seen = {}
    for L in SLICE_L:
        ref, tol = analysis(L, dtype, N)
        for operand, outs in SLICE_SEEN_IN.items():
            bad = defective(L, dtype, N, defect, operand)
            for k in outs:
                seen[(L, operand, k)] = float(_ratio(bad[k], ref[k], tol[k]).max())
    print(defect, N, NAME[dtype], round(min(seen.values()), 1))
    assert all(v > 4.0 for v in seen.values()), (defect, N, NAME[dtype], {k: v for k, v in seen.items() if v <= 4.0})
