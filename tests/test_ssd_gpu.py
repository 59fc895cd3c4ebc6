"""K6 / K6b (csrc/ssd.hip, csrc/ssd_bwd.hip: the Mamba-2 single-chunk SSD pair on the matrix pipe) per element against fp64, where the
state remembers.

The kernels are called through hip_ops.ssd_fwd / ssd_bwd.  The reference is the dual form the kernel headers state (ssd.hip:6-8,
ssd_bwd.hip:4-10), written as fp64 matmuls per (sequence, head) on the CPU from the rounded 16-bit inputs (`_dual`):
    dt = softplus(raw + bias),  s = A cumsum(dt),  M = exp(s_l - s_i) [i <= l],  W = (C B^T) .* M .* dt_i,  Y = W X + D X,  out = Y silu(z)
It is pinned once to the sequential restatement oracle/mamba2_ref.ssd_scan_ref (1e-12, CPU test); the backward references are fp64
autograd through that same function.  `_manual` restates the gradients in closed form (ssd_bwd.hip:6-10); with no rounding it equals
autograd (CPU test), with rounding where the kernel rounds it is the emulation the bounds are checked against, and with a defect
switched on it is what the bounds must be able to tell from the reference.

Inputs.  Four heads, each held in one regime by A_h, dt_bias_h and the level of the raw dt (dt_tok is 16-bit, token order, shared by
the directions); the level is multiplied by exp(0.3 randn) per token:
    slow  A = -1    dt ~ 0.003   log-decay over 224 steps ~ -0.7: every tile pair matters
    mid   A = -4    dt ~ 0.02    ~ -2.6 per tile
    fast  A = -16   dt ~ 0.1     the init corner: alpha * gamma underflows while the diagonal tile must not
    ends  A = -0.3  raw + bias ~ -12 (series branch of softplus_f, dt ~ 6e-6), every 40th token raw + bias ~ 25 (>= 20.5: the identity
          branch, a reset by e^-7.5); the backward's sigmoid(raw + bias) runs at the same two ends
x, B, C, z, dout are randn rounded to the dtype.  z / dt are gathered through one random row table per direction and out / dout go
through ANOTHER one (the kernels take the two tables separately), 1-3 directions, batch_per_dir 1 and 2.

Bounds.  u = unit roundoff of the I/O dtype (UNIT), T = absolute error of one rounding in the subnormal range (TINY: 2^-24 for fp16,
a spacing, twice the half-spacing that round-to-nearest gives; 2^-120 for bf16, whose range is fp32's), EPS32 = 2^-24.  One rounding of v
to 16 bits errs by at most u |v| + T.  None of the constants below is taken from a measured error.  An S-form is the reference
expression with every operand replaced by its absolute value (absolute values INSIDE the contractions), in fp64; all of them are
matmuls of the non-negative [L, L] matrices
    Gabs = |C| |B|^T,   Rabs = |gY| |X|^T (gY = dout silu(z)),   Mdt = M .* dt_i,   Wabs = Gabs .* Mdt,   dGabs = Rabs .* Mdt,   Vabs = Rabs .* Gabs .* M

fp32 part, C32[l, i]: relative error of the fp32 value of M[l, i] dt_i and of the sums it enters.
  * dt = softplus_f(x), x = raw + bias (dm_common.h:296-302).  e = exp2(x LOG2E): the product and the constant round (2 |x| EPS32 on e),
    v_exp_f32 is 1 ulp (2 EPS32).  Series branch (e < 2^-12): e (1 - e / 2), truncation < 2^-24 / 3: (2 |x| + 6) EPS32.  Middle branch:
    1 + e rounds (EPS32 absolute on the logarithm) and v_log_f32 is 1 ulp, taken for an argument in [1, 2) and a result
    near 0 as one more EPS32 ABSOLUTE, then two relative ulps: eps_dt = (2 / dt + 2 |x| + 10) EPS32 -- 4e-5 at dt = 0.003: log(1 + e) loses
    the small dt, which the model's slow heads have.  Identity branch: exact.  The backward's sigmoid_f: (2 |x| + 10) EPS32.
  * s2 = (A LOG2E dt) summed by an 8-step Hillis-Steele scan (forward; the backward's block scan is 6 + 3 additions of cumsum(dt), then
    one product): every partial sum has the sign of A, so each s2 errs by at most 10 EPS32 |s2|; M is exp2 of differences of s2
    values and tile-boundary values m_t that CANCEL exactly (the same fp32 number is added and subtracted), each difference rounds
    once more: 12 EPS32 (|s_l| + |s_i|) on M (natural-log units: ln 2 |s2| = |s|).  The errors of the dt values themselves enter both prefix
    sums alike: |A| sum_{i < j <= l} eps_dt_j dt_j.  This is the term that matters on the fast head, where |s| reaches hundreds.
  * three v_exp_f32, the products between them, the 16-term state sum and the sum over the keys (twice the term count, as in
    test_gemm_gpu.py, for the matrix pipe's internal adder): K0 EPS32 with K0 = 72 + 2 (l + 1) in the forward and a flat
    256 + 4 L in the backward (64-term R, the sums over positions, the block prefix sums, the sums over heads and sequences).
    C32[l, i] = EPS32 (12 (|s_l| + |s_i|) + K0) + |A| sum_{i < j <= l} eps_dt_j dt_j + eps_dt_i

Forward (ssd.hip).  Three 16-bit roundings on an off-diagonal pair: the scaled B rows b^ = rnd(B dt_i gamma_i) (:127), the scaled C
rows c^ = rnd(C alpha_l) (:190), the score tile rnd(g delta) (:207); two on a diagonal pair (rnd(B dt_i) :223, the tile :238-239; the
masked entries are exact zeros).  With a = |B| dt gamma, c = |C| alpha:  |b^ c^ - true| <= ((1 + u)^2 - 1) a c + T (1 + u)(a + c) + T^2, the
tile rounding adds u |g delta| + T, so per pair
    E[l, i] = ((1 + u)^3 - 1 + C32) Wabs + T ((1 + u)^2 (P1 sum_n |B_in| + P2 sum_n |C_ln|) + 1 + 17 T)
    P1 = delta gamma_i dt_i, P2 = delta alpha_l off the diagonal tile;  P1 = M dt_i, P2 = M on it       (the T part is what fp16 pays for
    dt ~ 6e-6: B dt is a subnormal there)
    |out - ref| <= |silu z| (E |X|)(1 + u)(1 + c_z) + 4 EPS32 |silu z| (Wabs |X| + |D X|) + (u + c_z) |ref| + T,    c_z = (2 |z| + 12) EPS32
The last line is the epilogue (:272-274): + D x and the gate in fp32 (silu_f: one v_exp_f32, one v_rcp_f32), one rounding of the result.
First order: 3 u S_l + u |ref_l| with S_l = (Wabs |X|)_l.

Backward (ssd_bwd.hip).  16-bit roundings: gY = rnd(dout silu(z)) (:159; dD uses the unrounded value, :157); the W tile rnd(G Mdt)
(:250 T orientation, :362 N); the dG tile rnd(R Mdt) (:251, :363); the outputs dz (:302) and dx (:405).  The one-hot products
(:223-225, :336-338) multiply by 1.0 and are exact; G and R are fp32 sums of exact products; the row / column sums of V (:249, :361) take
the fp32 values before the tile is rounded; dB / dC / d dt / dA / dD / d dt_bias leave in fp32.  With dg = u |gY| + T (error of the
stored gY), dR = dg |X|^T:
    dz        1 + 1 roundings   |dout silu'(z)|_abs ((u + C32) Wabs + T) |X| (1 + u) + (u + c_z) |ref| + T      (silu' is computed as
                                sg (1 + z (1 - sg)), which cancels near z = -1.28: its error is relative to sg (1 + |z| (1 - sg)))
    dx        2 + 1             ((u + C32) Wabs + T)^T (|gY| (1 + u) + T) + Wabs^T dg + |D| dg, times (1 + u), + u |ref| + T
    dB, dC    2                 sum over heads of (u (Rabs + dR) Mdt + dR Mdt + C32 dGabs + T)^T |C|   (dC: no transpose, |B|)
    d raw dt  1                 F(dR Gabs M + C32 Vabs) + c_sig F(Vabs),  F(V)_i = sig_i (colsum_i V + |A| sum_{l >= i} (V dt + dt colsum V)_l):
                                the reverse cumulative sum of d s is an fp32 block scan, inside K0
    dA, d dt_bias  1            sums over all positions, where an S-form is thousands of times the error.  Both are LINEAR in gY:
                                dA = sum_li V_li dt_i (cum_l - cum_i),  d dt_bias = sum_li V_li (sig_i + A dt_i (csig_l - csig_i)), V = (gY X^T) G M,
                                so the stored gY costs exactly sum_lp dg_lp |((G M Cf) X)_lp| with the SIGNED coefficient Cf; the fp32 part
                                is the S-form F / cum-weighted sum of M (|R| |G| (C32 + (256 + L) EPS32) + EPS32 (32 Gabs |R| + 128 Rabs |G|)):
                                signed R and G per pair, their own 64- and 16-term sums apart.  (The two orientations compute M
                                differently, so row sums and column sums of V do not cancel in fp32 as they do in the formula.)
    dD        0                 EPS32 (2 max|z| + 12 + 74 + S) sum |gY| |X|: 64 sequential terms per thread, the wave and block sums, S sequences

CPU tests (no GPU needed).  Every bound is checked against its own emulation (fp64 arithmetic, rounding only at the places listed):
ratio <= 0.5 for the fp32 outputs and for `out` before its last rounding, <= 1 where ONE rounding that the bound charges in full is
the whole error (test_bounds_hold_for_the_emulation_with_margin says which).  The defects of `DEFECTS` applied to the fp64 reference
must exceed 4 x the bound on the cases named for each; defect 7 (dA without the far pairs) is named at bf16 for L = 196 only.

Buffers.  x | B | C are column blocks of one NaN-padded buffer; out, dx, dz (and dout, read) are views with sentinel rows before and
after and sentinel columns beside them, NaN inside: every element must be written, the frame must survive bit for bit.  hip_ops.ssd_bwd
allocates dz itself, so the framed dz goes through a hand-built dm_ssd_bwd_args, which also serves the C-ABI check that the backward
refuses L = 197 .. 224 while the forward takes them.
"""
import ctypes
import functools
import math

import pytest
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
NAME = {BF16: "bf16", F16: "f16"}
EPS32 = 2.0 ** -24
UNIT = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
TINY = {BF16: 2.0 ** -120, F16: 2.0 ** -24}
H, P, N, TILE = 4, 64, 16, 32
DIN = H * P
A_H = torch.tensor([-1.0, -4.0, -16.0, -0.3], dtype=torch.float64)
BIAS_H = torch.tensor([0.25, -0.5, 0.75, -1.0], dtype=torch.float64)
D_H = torch.tensor([0.5, -1.0, 1.5, 0.25], dtype=torch.float64)
DT_LEVEL = torch.tensor([0.003, 0.02, 0.1], dtype=torch.float64)
HEAD = ["slow", "mid", "fast", "ends"]
DM_OK, DM_ERR_ARG = 0, -1
NAN = float("nan")
SENT = 7.0
WORST = {}                                             # (what, dtype) -> worst |got - ref| / bound, printed per test

# L -> (directions, batch_per_dir); S = directions * batch_per_dir <= 6
FWD_L = {1: (1, 1), 31: (2, 1), 32: (1, 2), 33: (3, 1), 65: (2, 2), 97: (3, 2), 196: (3, 2), 223: (1, 1), 224: (2, 1)}
BWD_L = {1: (1, 1), 32: (1, 2), 33: (3, 1), 65: (2, 2), 97: (3, 2), 129: (2, 1), 196: (3, 2)}
GRADS = ["dx", "dz", "dB", "dC", "ddt", "dA", "dD", "dbias"]


def _softplus(x):
    from oracle.mamba_ref import softplus_ref

    return softplus_ref(x)


def _silu(z):
    return z * torch.sigmoid(z)


# =====================================================================================================================================
# inputs
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def _inputs(L, dtype):
    """Host tensors of one case (16-bit where the kernel reads 16 bits), the same for the forward and the backward."""
    ndir, bpd = BWD_L[L] if L in BWD_L else FWD_L[L]
    assert L not in FWD_L or L not in BWD_L or FWD_L[L] == BWD_L[L]
    S = ndir * bpd
    g = torch.Generator().manual_seed(1000 * L + (1 if dtype == F16 else 0))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    xBC = rn(S, L, DIN + 2 * N).to(dtype)
    z = rn(bpd, L, DIN).to(dtype)
    dout = rn(S, L, DIN).to(dtype)
    pre = torch.log(torch.expm1(DT_LEVEL * torch.exp(0.3 * rn(bpd, L, 3))))             # raw + bias of the three softplus-middle heads
    ends = -12.0 + 0.3 * rn(bpd, L)                                                      # series branch: dt = e^x, so exp(0.3 randn) on dt is + 0.3 randn
    spike = (torch.arange(L)[None] + 7 * torch.arange(bpd)[:, None]) % 40 == 5
    ends = torch.where(spike, (25.0 * torch.exp(0.3 * rn(bpd, L))).clamp_min(20.5), ends)
    dt_tok = (torch.cat([pre, ends[..., None]], -1) - BIAS_H).to(dtype)
    zperm = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)])
    operm = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)])
    return dict(L=L, dtype=dtype, ndir=ndir, bpd=bpd, S=S, xBC=xBC, z=z, dout=dout, dt_tok=dt_tok, zperm=zperm, operm=operm)


def _seq(c, s, table0=False):
    """fp64 operands of sequence s in SCAN order: x [L, H, P], B, C [L, N], raw + bias [L, H], z, dout [L, H, P], and its two row tables.
    table0: every direction reads direction 0's tables (defect 5)."""
    k, b = divmod(s, c["bpd"])
    zi, oi = c["zperm"][0 if table0 else k], c["operm"][0 if table0 else k]
    L = c["L"]
    d = lambda t: t.double()
    x = d(c["xBC"][s, :, :DIN]).view(L, H, P)
    return dict(x=x, B=d(c["xBC"][s, :, DIN:DIN + N]), C=d(c["xBC"][s, :, DIN + N:]), pre=d(c["dt_tok"][b])[zi] + BIAS_H,
                z=d(c["z"][b])[zi].view(L, H, P), dout=d(c["dout"][s])[oi].view(L, H, P), zi=zi, oi=oi)


# =====================================================================================================================================
# the operator in fp64: dual form, closed-form gradients, emulation, defects
# =====================================================================================================================================
def _decay(s, L, defect=None):
    """M[h, l, i] = exp(s_l - s_i) [i <= l] from s [L, H]; defects 1-3 act here."""
    sT = s.t()
    idx = torch.arange(L)
    tl = idx // TILE
    keep = idx[:, None] >= idx[None, :]
    if defect == "diag_mask":
        keep = idx[:, None] > idx[None, :]
    far = (tl[:, None] - tl[None, :]) >= 2
    if defect == "drop_far":
        keep = keep & ~far
    M = torch.exp((sT[:, :, None] - sT[:, None, :]).masked_fill(~keep, -math.inf))
    if defect == "delta_prev":                                       # delta = exp(m_lt - m_it): one key tile's decay too many
        m = torch.cat([torch.zeros(H, 1, dtype=s.dtype), sT[:, TILE - 1::TILE], sT[:, -1:]], 1)          # m_t, t = 0 .. (padded at the end)
        step = (m[:, 1:] - m[:, :-1])[:, tl]                         # m_{it+1} - m_it per key
        M = torch.where(far, M * torch.exp(step)[:, None, :], M)
    return M


def _dual(q, A, D, bias_shift=None, defect=None):
    """out [L, H, P] in scan order (autograd-capable).  q: dict of _seq; A, D: [H]."""
    L = q["x"].shape[0]
    Au, pre = A, q["pre"] if bias_shift is None else q["pre"] + bias_shift
    if defect == "prev_head_A":
        Au = A.roll(1)
    dt = _softplus(pre)
    M = _decay(Au * dt.cumsum(0), L, defect)
    W = (q["C"] @ q["B"].t())[None] * M * dt.t()[:, None, :]
    Y = torch.einsum("hli,ihp->lhp", W, q["x"]) + D[None, :, None] * q["x"]
    return Y * _silu(q["z"])


def _manual(q, A, D, rnd=None, defect=None):
    """Forward and every gradient of one sequence in closed form (ssd_bwd.hip:6-10), scan order.  rnd: the 16-bit rounding applied
    where the KERNELS round (None: none, the fp64 value); the forward is then ssd.hip's factorised form.  defect: 'no_A_term', 'dA_near'."""
    r = rnd if rnd is not None else (lambda v: v)
    L = q["x"].shape[0]
    x, Bm, Cm, z, do = q["x"], q["B"], q["C"], q["z"], q["dout"]
    dt = _softplus(q["pre"])
    sig = torch.where(q["pre"] > 20.0, torch.ones_like(dt), torch.sigmoid(q["pre"]))
    cum = dt.cumsum(0)
    s = A * cum
    M = _decay(s, L)
    Mdt = M * dt.t()[:, None, :]
    G = (Cm @ Bm.t())[None]
    sg = torch.sigmoid(z)
    # ---- forward as ssd.hip rounds it ----
    if rnd is None:
        Wf = G * Mdt
    else:
        idx = torch.arange(L)
        tl = idx // TILE
        sT = s.t()
        m = torch.cat([torch.zeros(H, 1, dtype=s.dtype), sT[:, TILE - 1::TILE], sT[:, -1:]], 1)
        alpha = torch.exp(sT - m[:, tl])                                                 # [H, L]
        gamma = torch.exp(m[:, tl + 1] - sT)
        delta = torch.exp(m[:, tl][:, :, None] - m[:, tl + 1][:, None, :])              # [H, l, i] (used where tile_i < tile_l)
        bh = r(Bm[None] * (dt.t() * gamma)[:, :, None])                                  # [H, L, N]
        ch = r(Cm[None] * alpha[:, :, None])
        off = (tl[:, None] > tl[None, :])[None]
        Woff = r(torch.einsum("hln,hin->hli", ch, bh) * torch.where(off, delta, torch.zeros_like(delta)))
        Wdiag = r(torch.einsum("ln,hin->hli", Cm, r(Bm[None] * dt.t()[:, :, None])) * M)
        Wf = torch.where(off, Woff, torch.where((tl[:, None] == tl[None, :])[None], Wdiag, torch.zeros_like(Wdiag)))
    out_pre = (torch.einsum("hli,ihp->lhp", Wf, x) + D[None, :, None] * x) * _silu(z)
    # ---- backward as ssd_bwd.hip rounds it ----
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
    rs = (V * dt.t()[:, None, :]).sum(2)                                                 # [H, L]
    cs = V.sum(1)
    ds = rs - dt.t() * cs
    rc = ds.flip(1).cumsum(1).flip(1)
    ddt = cs + (0.0 if defect == "no_A_term" else A[:, None] * rc)
    if defect == "dA_near":
        tl = torch.arange(L) // TILE
        Vn = V * ((tl[:, None] - tl[None, :]) < 2)[None]
        ds = (Vn * dt.t()[:, None, :]).sum(2) - dt.t() * Vn.sum(1)
    draw = (ddt * sig.t()).t()                                                           # [L, H]
    return dict(out=r(out_pre), dx=r(dx_pre), dz=r(dz_pre), out_pre=out_pre, dx_pre=dx_pre, dz_pre=dz_pre, dB=dB.sum(0), dC=dC.sum(0), ddt=draw, dA=(ds * cum.t()).sum(1), dD=(gy * x).sum((0, 2)),
                dbias=draw.sum(0))


def _bounds(q, A, D, dtype, ref_out, ref):
    """Per-element bounds of the module docstring for one sequence (scan order); ref: the fp64 gradients (None: forward only)."""
    u, T = UNIT[dtype], TINY[dtype]
    L = q["x"].shape[0]
    x, Bm, Cm, z, do, pre = q["x"].abs(), q["B"].abs(), q["C"].abs(), q["z"], q["dout"], q["pre"]
    xs = q["x"]
    dt = _softplus(pre)
    cum = dt.cumsum(0)
    s = A * cum
    sT, dtT = s.t(), dt.t()
    idx = torch.arange(L)
    tl = idx // TILE
    causal = (idx[:, None] >= idx[None, :])[None]
    M = _decay(s, L)
    Mdt = M * dtT[:, None, :]
    middle = (pre <= 20.0) & (torch.exp(pre) >= 2.0 ** -12)
    eps_dt = EPS32 * (torch.where(middle, 2.0 / dt, torch.zeros_like(dt)) + 2 * pre.abs() + 10)          # [L, H]
    errs = (A.abs() * (eps_dt * dt).cumsum(0)).t()                                                      # [H, L]
    C32 = EPS32 * 12 * (sT.abs()[:, :, None] + sT.abs()[:, None, :]) + (errs[:, :, None] - errs[:, None, :]).clamp_min(0) + eps_dt.t()[:, None, :]
    Gabs = (Cm @ Bm.t())[None]
    Wabs = Gabs * Mdt
    cz = EPS32 * (2 * z.abs() + 12)
    silu = _silu(z).abs()
    mm = lambda E, v: torch.einsum("hli,ihp->lhp", E, v)
    # ---- forward ----
    m = torch.cat([torch.zeros(H, 1, dtype=s.dtype), sT[:, TILE - 1::TILE], sT[:, -1:]], 1)
    alpha, gamma = torch.exp(sT - m[:, tl]), torch.exp(m[:, tl + 1] - sT)
    delta = torch.exp((m[:, tl][:, :, None] - m[:, tl + 1][:, None, :]).clamp_max(0))
    off = (tl[:, None] > tl[None, :])[None]
    P1 = torch.where(off, delta * (gamma * dtT)[:, None, :], Mdt)
    P2 = torch.where(off, delta * alpha[:, :, None], M)
    K0f = EPS32 * (72 + 2 * (idx + 1.0))[None, :, None]
    Ef = ((1 + u) ** 3 - 1 + C32 + K0f) * Wabs + T * ((1 + u) ** 2 * (P1 * Bm.sum(1)[None, None, :] + P2 * Cm.sum(1)[None, :, None]) + 1 + 17 * T) * causal
    Dx = D.abs()[None, :, None] * x
    tol = dict(out=silu * mm(Ef, x) * (1 + u) * (1 + cz) + 4 * EPS32 * silu * (mm(Wabs, x) + Dx) + (u + cz) * ref_out.abs() + T)
    if ref is None:
        return tol
    # ---- backward ----
    sg = torch.sigmoid(z)
    sig = torch.where(pre > 20.0, torch.ones_like(dt), torch.sigmoid(pre))
    gy = (do * _silu(z)).abs()
    dg = (u + cz) * gy + T
    C32b = C32 + EPS32 * (256 + 4 * L)
    Rabs = torch.einsum("lhp,ihp->hli", gy, x) * causal
    dR = torch.einsum("lhp,ihp->hli", dg, x) * causal
    EW = (u + C32b) * Wabs + T * causal
    spabs = sg * (1 + z.abs() * (1 - sg))
    tol["dz"] = do.abs() * spabs * (mm(EW, x) * (1 + u) + (cz + 4 * EPS32) * (mm(Wabs, x) + Dx)) + (u + cz) * ref["dz"].abs() + T
    tol["dx"] = (torch.einsum("hli,lhp->ihp", EW, gy * (1 + u) + T) + torch.einsum("hli,lhp->ihp", Wabs, dg) + D.abs()[None, :, None] * dg
                 + 4 * EPS32 * D.abs()[None, :, None] * gy) * (1 + u) + u * ref["dx"].abs() + T
    EdG = u * (Rabs + dR) * Mdt + dR * Mdt + C32b * Rabs * Mdt + T * causal
    tol["dB"] = torch.einsum("hli,ln->in", EdG, Cm)
    tol["dC"] = torch.einsum("hli,in->ln", EdG, Bm)
    Vabs = Rabs * Gabs * M
    Veps = dR * Gabs * M + C32b * Vabs
    csig = EPS32 * (2 * pre.abs() + 10).t()
    inner = lambda V: (V @ dtT[:, :, None]).squeeze(2) + dtT * V.sum(1)                                   # [H, L]: |d s| form
    F = lambda V: sig.t() * (V.sum(1) + A.abs()[:, None] * inner(V).flip(1).cumsum(1).flip(1))
    tol["ddt"] = (F(Veps) + csig * F(Vabs)).t()
    # the reductions over positions: exact sensitivities to the stored gY, signed R and G in the fp32 part (module docstring)
    Rs = torch.einsum("lhp,ihp->hli", do * _silu(z), xs) * causal
    Gs = (q["C"] @ q["B"].t())[None]
    E32V = M * (Rs.abs() * Gs.abs() * (C32 + EPS32 * (256 + L)) + EPS32 * (32 * Gabs * Rs.abs() + 128 * Rabs * Gs.abs()))
    red = lambda Cf: (dg * torch.einsum("hli,ihp->lhp", Gs * M * Cf, xs).abs()).sum((0, 2))
    cumT, sigT = cum.t(), sig.t()
    csum = sigT.cumsum(1)
    tol["dA"] = red(dtT[:, None, :] * (cumT[:, :, None] - cumT[:, None, :])) + (inner(E32V) * cumT).sum(1)
    tol["dbias"] = (red(sigT[:, None, :] + A[:, None, None] * dtT[:, None, :] * (csum[:, :, None] - csum[:, None, :]))
                    + (F(E32V) + csig * F(Rs.abs() * Gs.abs() * M)).sum(1))
    tol["dD"] = EPS32 * (2 * float(z.abs().max()) + 12 + 74) * (gy * x).sum((0, 2))
    return tol


@functools.lru_cache(maxsize=None)
def _analysis(L, dtype, backward):
    """Reference (fp64; gradients by autograd through _dual), bounds and emulation of one case, in the KERNELS' output layout:
    out / dz / d raw dt rows through the row tables, dx / dB / dC in scan order, dA / dD / d dt_bias summed over the sequences."""
    c = _inputs(L, dtype)
    S = c["S"]
    rnd = lambda v: v.to(dtype).double()
    keys = ["out"] + (GRADS if backward else [])
    ref, tol, emu = ({k: [] for k in keys} for _ in range(3))
    A = A_H.clone().requires_grad_(backward)
    D = D_H.clone().requires_grad_(backward)
    shift = torch.zeros(H, dtype=torch.float64, requires_grad=backward)
    for s in range(S):
        q = _seq(c, s)
        leaves = {}
        if backward:
            for k in ("x", "B", "C", "pre", "z"):
                leaves[k] = q[k].clone().requires_grad_(True)
        out = _dual({**q, **leaves}, A, D, shift if backward else None)
        r = None
        if backward:
            ga, gd, gs = (None if t.grad is None else t.grad.clone() for t in (A, D, shift))
            (out * q["dout"]).sum().backward()
            part = lambda t, g0: t.grad.clone() if g0 is None else t.grad - g0
            r = dict(dx=leaves["x"].grad, dz=leaves["z"].grad, dB=leaves["B"].grad, dC=leaves["C"].grad, ddt=leaves["pre"].grad,
                     dA=part(A, ga), dD=part(D, gd), dbias=part(shift, gs))
        out = out.detach()
        t = _bounds(q, A_H, D_H, dtype, out, r)
        e = _manual(q, A_H, D_H, rnd)
        r = dict(out=out, **(r or {}))
        for k in keys + [k + "_pre" for k in keys if k in ("out", "dx", "dz")]:
            for dst, src in ((ref, r), (tol, t), (emu, e)):
                if k not in src:
                    continue
                v = src[k]
                if k in ("out", "out_pre"):
                    v = torch.empty_like(v).index_copy_(0, q["oi"], v)                   # step l lands in row out_row_index[l]
                elif k in ("dz", "dz_pre", "ddt"):
                    v = torch.empty_like(v).index_copy_(0, q["zi"], v)                   # ... z_row_index[l]
                dst.setdefault(k, []).append(v.reshape(L, -1) if v.dim() == 3 else v)
    red = lambda d, k: torch.stack(d[k]).sum(0) if k in ("dA", "dD", "dbias") else torch.stack(d[k])
    ref, tol, emu = ({k: red(d, k) for k in d} for d in (ref, tol, emu))
    for k in ("dA", "dD", "dbias"):
        if backward:                                                                     # the sum over the sequences: S fp32 additions
            tol[k] = tol[k] * (1 + S * EPS32) + S * EPS32 * ref[k].abs()
    return ref, tol, emu


def _an(L, dtype):
    return _analysis(L, dtype, L in BWD_L)


def _defective(L, dtype, defect):
    """{output: tensor} of the fp64 operator with one defect, in the layout of _analysis."""
    c = _inputs(L, dtype)
    res = {}
    for s in range(c["S"]):
        q = _seq(c, s, table0=(defect == "table0"))
        if defect in ("no_A_term", "dA_near"):
            m = _manual(q, A_H, D_H, None, defect)
            res.setdefault("ddt", []).append(torch.empty_like(m["ddt"]).index_copy_(0, q["zi"], m["ddt"]))
            res.setdefault("dA", []).append(m["dA"])
        else:
            o = _dual(q, A_H, D_H, defect=defect)
            res.setdefault("out", []).append(torch.empty_like(o).index_copy_(0, q["oi"], o).reshape(L, -1))
    return {k: torch.stack(v).sum(0) if k == "dA" else torch.stack(v) for k, v in res.items()}


def _ratio(got, ref, tol):
    r = (got.double() - ref).abs() / tol
    return r.nan_to_num(nan=1e30)


def _head_of(k, r):
    """Worst ratio per head for the outputs that have a head axis (diagnostics in the failure message)."""
    if k in ("out", "dx", "dz"):
        return [float(r.reshape(*r.shape[:-1], H, P)[..., h, :].max()) for h in range(H)]
    if k == "ddt":
        return [float(r[..., h].max()) for h in range(H)]
    if k in ("dA", "dD", "dbias"):
        return [float(v) for v in r]
    return [float(r.max())]


def _check(what, dtype, got, ref, tol):
    r = _ratio(got, ref, tol)
    worst = float(r.max())
    WORST[(what, NAME[dtype])] = max(WORST.get((what, NAME[dtype]), 0.0), worst)
    assert worst <= 1.0, f"{what} {NAME[dtype]}: worst |got - ref| / bound {worst:.3f}; per head {_head_of(what, r)}"


def _report():
    """The figures measured so far (shown by pytest -s / -rP)."""
    for k in sorted(WORST):
        print(f"worst |got - ref| / bound  {k[0]:6s} {k[1]:5s}: {WORST[k]:.4f}")


# =====================================================================================================================================
# CPU: the reference, the emulation against the bounds, the defects against the bounds
# =====================================================================================================================================
def test_dual_form_equals_the_sequential_oracle():
    """_dual against oracle/mamba2_ref.ssd_scan_ref (the sequential recurrence) at L = 65 (three tiles), all four regimes: 1e-12 of the
    largest output; _manual without rounding equals _dual and fp64 autograd through it."""
    from oracle.mamba2_ref import ssd_scan_ref

    L = 65
    c = _inputs(L, BF16)
    ref, _, _ = _an(L, BF16)
    for s in range(c["S"]):
        q = _seq(c, s)
        y = ssd_scan_ref(q["x"].reshape(1, L, DIN), _softplus(q["pre"])[None], A_H, q["B"][None], q["C"][None], D_H, P)[0]
        want = (y.view(L, H, P) * _silu(q["z"]))
        got = _dual(q, A_H, D_H)
        assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
        m = _manual(q, A_H, D_H)
        assert float((m["out"] - got).abs().max()) <= 1e-12 * float(want.abs().max())
        inv = lambda v, t: v[t]                                                          # kernel layout -> scan order
        for k in ("dx", "dz", "dB", "dC", "ddt"):
            r = ref[k][s]
            r = inv(r, q["zi"]) if k in ("dz", "ddt") else r
            g = m[k].reshape(r.shape)
            assert float((g - r).abs().max()) <= 1e-10 * float(r.abs().max()), k
    tot = {k: sum(_manual(_seq(c, s), A_H, D_H)[k] for s in range(c["S"])) for k in ("dA", "dD", "dbias")}
    for k, v in tot.items():
        assert float((v - ref[k]).abs().max()) <= 1e-10 * float(ref[k].abs().max()), k


def test_inputs_reach_every_regime():
    """What the module docstring promises of the inputs: the slow head keeps half of its state over 224 steps, the fast head's
    alpha * gamma underflows fp32, the ends head runs the series and the identity branch of softplus_f (and neither of the others)."""
    c = _inputs(224, BF16)
    q = _seq(c, 0)
    dt = _softplus(q["pre"])
    s = A_H * dt.cumsum(0)
    assert float(s[-1, 0]) > math.log(0.4) and -4.0 < float(s[31, 1]) < -1.5
    assert float((s[63, 2] - s[32, 2]) + (s[31, 2] - s[0, 2])) * math.log2(math.e) < -126          # alpha_63 * gamma_0 < 2^-126
    e = torch.exp(q["pre"][:, 3])
    assert bool(((e < 2.0 ** -12) | (q["pre"][:, 3] > 20.0)).all()) and int((q["pre"][:, 3] > 20.0).sum()) >= 4
    assert bool(((torch.exp(q["pre"][:, :3]) >= 2.0 ** -12) & (q["pre"][:, :3] < 20.0)).all())


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_bounds_hold_for_the_emulation_with_margin(dtype):
    """Every derived bound against its own emulation (fp64, rounded where the kernels round), every listed L: worst ratio <= 0.5 for
    the fp32 outputs (dB, dC, d raw dt, dA, dD, d dt_bias) and for `out` before its last rounding.  A worst-case bound cannot keep a
    factor of two over ONE rounding that it charges in full, and three things here are one rounding: the last rounding of out / dx /
    dz (u |ref|, reached by a value just above a power of two; at L = 1 out is D x silu(z) but for one product), the stored gY in
    dx = .. + D gY, and W_ll x_l in dz on the fast head, where the next key is down by e^-1.6.  Those (out, dx, dz rounded; dx, dz
    before the last rounding: 0.50 and 0.56 here) are held to <= 1."""
    worst = {}
    for L in sorted(set(FWD_L) | set(BWD_L)):
        ref, tol, emu = _an(L, dtype)
        for k in emu:
            kr = k[:-4] if k.endswith("_pre") else k
            r = _ratio(emu[k], ref[kr], tol[kr])
            worst[k] = max(worst.get(k, 0.0), float(r.max()))
            assert float(r.max()) <= (1.0 if k in ("out", "dx", "dz", "dx_pre", "dz_pre") else 0.5), (k, L, NAME[dtype], float(r.max()), _head_of(kr, r))
    print({k: round(v, 4) for k, v in worst.items()})


# defect -> (output it is looked for in, the L it must show at)
DEFECTS = {
    "drop_far": ("out", [65, 97, 196, 223, 224]),                    # 1. keys more than one tile back dropped
    "delta_prev": ("out", [65, 97, 196, 223, 224]),                  # 2. far-tile delta from m_it instead of m_{it+1}
    "diag_mask": ("out", [1, 31, 32, 33, 65, 97, 196, 223, 224]),       # 3. diagonal mask i < l
    "prev_head_A": ("out", [31, 32, 33, 65, 97, 196, 223, 224]),        # 4. head h with the A of head h - 1
    "table0": ("out", [31, 33, 65, 97, 196, 224]),           # 5. direction k with direction 0's row tables (every L with 2+ directions)
    "no_A_term": ("ddt", [32, 33, 65, 97, 129, 196]),        # 6. d dt without A * sum_{l >= i} d s_l
    "dA_near": ("dA", {F16: [97, 129, 196], BF16: [196]}),   # 7. dA without the pairs two or more tiles apart.  bf16 at L = 97 / 129: the
}                                                            #    far pairs' share of dA is 0.3 / 2.5 bounds (8 bits in gY, summed over 64 L terms)


@pytest.mark.parametrize("defect", list(DEFECTS))
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_bounds_tell_each_defect_from_the_reference(dtype, defect):
    """The test can fail: each defect, applied to the fp64 reference, leaves at least one element more than 4 x its bound away, at
    every L named for it."""
    what, Ls = DEFECTS[defect]
    Ls = Ls[dtype] if isinstance(Ls, dict) else Ls
    seen = {}
    for L in Ls:
        ref, tol, _ = _an(L, dtype)
        bad = _defective(L, dtype, defect)[what]
        seen[L] = float(_ratio(bad, ref[what], tol[what]).max())
    print(defect, NAME[dtype], {L: round(v, 1) for L, v in seen.items()})
    assert all(v > 4.0 for v in seen.values()), (defect, NAME[dtype], seen)


# =====================================================================================================================================
# GPU
# =====================================================================================================================================
def _device_operands(gpu, c):
    L, S, dtype = c["L"], c["S"], c["dtype"]
    xb = torch.full((S, L + 4, DIN + 2 * N + 8), NAN, dtype=dtype, device=gpu)           # NaN rows before / after, NaN columns beside
    xb[:, 2:2 + L, :DIN + 2 * N] = c["xBC"].to(gpu)
    v = xb[:, 2:2 + L]
    tabs = dict(z_row_index=c["zperm"].int().to(gpu), out_row_index=c["operm"].int().to(gpu), batch_per_dir=c["bpd"])
    return xb, v[..., :DIN], v[..., DIN:DIN + N], v[..., DIN + N:DIN + 2 * N], c["dt_tok"].to(gpu), c["z"].to(gpu), tabs


def _framed(gpu, S, L, dtype):
    """[S, L, DIN] view with two sentinel rows before and after it and sentinel columns beside it; the view itself holds NaN."""
    buf = torch.full((S, L + 4, DIN + 8), SENT, dtype=dtype, device=gpu)
    view = buf[:, 2:2 + L, :DIN]
    view.fill_(NAN)
    return buf, view


def _frame_untouched(buf, L):
    chk = buf.clone()
    chk[:, 2:2 + L, :DIN] = SENT
    return bool((chk == SENT).all())


@pytest.mark.gpu
@pytest.mark.parametrize("L", sorted(FWD_L))
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_ssd_fwd_within_derived_bound(gpu, dtype, L):
    """dm_ssd_fwd per element within the forward bound of the module docstring; `out` is a view inside a sentinel frame that must
    survive bit for bit, every element of the view is written (it starts as NaN), the operands are read-only."""
    from diffma_amd import hip_ops

    c = _inputs(L, dtype)
    ref, tol, _ = _an(L, dtype)
    xb, x, Bm, Cm, dt_tok, z, tabs = _device_operands(gpu, c)
    xb0 = xb.clone()
    buf, view = _framed(gpu, c["S"], L, dtype)
    out = hip_ops.ssd_fwd(x, Bm, Cm, dt_tok, z, A_H.float().to(gpu), D_H.float().to(gpu), BIAS_H.float().to(gpu), out=view, **tabs)
    torch.cuda.synchronize()
    assert out.data_ptr() == view.data_ptr() and _frame_untouched(buf, L), "written outside out"
    assert torch.equal(xb.view(torch.int16), xb0.view(torch.int16)), "operands are read-only"
    _check("out", dtype, view.cpu().reshape(c["S"], L, DIN), ref["out"], tol["out"])
    _report()


@pytest.mark.gpu
@pytest.mark.parametrize("L", sorted(BWD_L))
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_ssd_bwd_within_derived_bounds(gpu, dtype, L):
    """dm_ssd_bwd: every gradient per element within its bound.  dx lands in the x columns of a NaN-filled [S, L + 4, DIN + 40] buffer
    (the mixer's layout: the B | C columns and the spare rows keep their NaN bit for bit)."""
    from diffma_amd import hip_ops

    c = _inputs(L, dtype)
    S = c["S"]
    ref, tol, _ = _an(L, dtype)
    xb, x, Bm, Cm, dt_tok, z, tabs = _device_operands(gpu, c)
    dxb = torch.full_like(xb, SENT)
    dxv = dxb[:, 2:2 + L, :DIN]
    dxv.fill_(NAN)
    dx, dz, dbc, ddt, dad = hip_ops.ssd_bwd(x, Bm, Cm, dt_tok, z, c["dout"].to(gpu), A_H.float().to(gpu), D_H.float().to(gpu),
                                            BIAS_H.float().to(gpu), dx_out=dxv, **tabs)
    torch.cuda.synchronize()
    chk = dxb.clone()
    chk[:, 2:2 + L, :DIN] = SENT
    assert dx.data_ptr() == dxv.data_ptr() and bool((chk == SENT).all()), "written outside dx"
    got = dict(dx=dxv.cpu(), dz=dz.cpu(), dB=dbc[..., :N].cpu(), dC=dbc[..., N:].cpu(), ddt=ddt.cpu(), dA=dad[0].cpu(), dD=dad[1].cpu(),
               dbias=dad[2].cpu())
    fails = []
    for k in GRADS:
        try:
            _check(k, dtype, got[k].reshape(ref[k].shape), ref[k], tol[k])
        except AssertionError as e:
            fails.append(str(e))
    _report()
    assert not fails, "\n".join(fails)


def _bwd_args(gpu, L, dtype, S=1, given=None, tabs=None):
    """A hand-built dm_ssd_bwd_args: zero operands and sentinel-filled outputs, each replaced by `given`'s view of that name."""
    z = lambda *s, dt=dtype: torch.zeros(*s, dtype=dt, device=gpu)
    f = lambda *s, dt=dtype: torch.full(s, SENT, dtype=dt, device=gpu)
    t = dict(x=z(S, L, DIN), B=z(S, L, N), C=z(S, L, N), dt=z(S, L, H), z=z(S, L, DIN), dout=z(S, L, DIN), dx=f(S, L, DIN), dz=f(S, L, DIN),
             A=torch.full((H,), -1.0, device=gpu), dBC=f(H, S, L, 32, dt=F32), ddt=f(S, L, H, dt=F32), dAD=f(S, 3, H, dt=F32))
    t.update(given or {})
    a = _lib().dm_ssd_bwd_args()
    a.nseq, a.batch_per_dir, a.seqlen, a.nheads, a.headdim, a.dstate = S, (tabs or {}).get("batch_per_dir", 0), L, H, P, N
    a.io_dtype, a.flags = (1 if dtype == BF16 else 2), 0
    a.x, a.B, a.C, a.dt, a.z, a.dout = (t[k].data_ptr() for k in ("x", "B", "C", "dt", "z", "dout"))
    a.A, a.dx, a.dz, a.dBC_part, a.ddt, a.dAD_part = (t[k].data_ptr() for k in ("A", "dx", "dz", "dBC", "ddt", "dAD"))
    if "D" in t:
        a.D, a.dt_bias = t["D"].data_ptr(), t["bias"].data_ptr()
    if tabs:
        a.z_row_index, a.out_row_index = tabs["z_row_index"].data_ptr(), tabs["out_row_index"].data_ptr()
    for k, v in (("x", "x"), ("B", "B"), ("C", "C"), ("z", "z"), ("do", "dout"), ("dx", "dx"), ("dz", "dz")):
        setattr(a, k + "_ss", t[v].stride(0))
        setattr(a, k + "_sl", t[v].stride(1))
    a.dt_sb, a.dt_sl = t["dt"].stride(0), t["dt"].stride(1)
    return a, t


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_ssd_bwd_dz_and_dx_land_in_framed_views(gpu, dtype):
    """The struct by hand (hip_ops.ssd_bwd allocates dz itself): dz and dx are views with sentinel rows before and after them and
    sentinel columns beside them, dout is read from such a view; L = 33 (a one-row last tile), three directions.  Both within
    their bounds, every element written, the frames bit for bit."""
    L = 33
    c = _inputs(L, dtype)
    S = c["S"]
    ref, tol, _ = _an(L, dtype)
    xb, x, Bm, Cm, dt_tok, z, tabs = _device_operands(gpu, c)
    dzb, dzv = _framed(gpu, S, L, dtype)
    dxb, dxv = _framed(gpu, S, L, dtype)
    dob, dov = _framed(gpu, S, L, dtype)
    dob.fill_(NAN)
    dov.copy_(c["dout"].to(gpu))
    keep = [A_H.float().to(gpu), D_H.float().to(gpu), BIAS_H.float().to(gpu)]
    a, t = _bwd_args(gpu, L, dtype, S, dict(x=x, B=Bm, C=Cm, dt=dt_tok, z=z, dout=dov, dx=dxv, dz=dzv, A=keep[0], D=keep[1], bias=keep[2]), tabs)
    lib = _lib().load()
    rc = int(lib.dm_ssd_bwd(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert rc == DM_OK, lib.dm_last_error().decode()
    torch.cuda.synchronize()
    assert _frame_untouched(dzb, L) and _frame_untouched(dxb, L), "written outside dz / dx"
    _check("dz", dtype, dzv.cpu(), ref["dz"], tol["dz"])
    _check("dx", dtype, dxv.cpu(), ref["dx"], tol["dx"])
    _check("ddt", dtype, t["ddt"].cpu(), ref["ddt"], tol["ddt"])
    _report()


def _lib():
    from diffma_amd import _lib as L

    return L


@pytest.mark.gpu
def test_ssd_bwd_refuses_what_only_the_forward_takes(gpu):
    """The forward takes L <= 224, the backward L <= 196: for L = 197 .. 224 dm_ssd_fwd_supported is 1, dm_ssd_bwd_supported is 0 and
    dm_ssd_bwd returns DM_ERR_ARG with a message of its own and writes nothing; at L = 196 the same struct is accepted."""
    L_ = _lib()
    lib = L_.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for code, dtype in ((1, BF16), (2, F16)):
        for L in range(197, 225):
            assert lib.dm_ssd_fwd_supported(L, P, N, code) == 1 and lib.dm_ssd_bwd_supported(L, P, N, code) == 0, L
        assert lib.dm_ssd_bwd_supported(196, P, N, code) == 1 and lib.dm_ssd_fwd_supported(225, P, N, code) == 0
        for L in (197, 224):
            a, t = _bwd_args(gpu, L, dtype)
            assert int(lib.dm_ssd_bwd(ctypes.byref(a), st)) == DM_ERR_ARG
            assert lib.dm_last_error().decode().startswith("dm_ssd_bwd: needs")
            torch.cuda.synchronize()
            assert all(bool((t[k] == SENT).all()) for k in ("dx", "dz", "dBC", "ddt", "dAD")), "a refused call wrote"
        a, t = _bwd_args(gpu, 196, dtype)
        assert int(lib.dm_ssd_bwd(ctypes.byref(a), st)) == DM_OK, lib.dm_last_error().decode()
        torch.cuda.synchronize()
        assert bool((t["dx"] == 0).all()) and bool((t["ddt"] == 0).all())               # zero operands: zero gradients, all written


@pytest.mark.gpu
def test_mamba2_mixer_past_the_backward_limit_trains_on_the_scan_pair(gpu, monkeypatch):
    """L = 200 is inside the forward's range and outside the backward's: a call that needs gradients must run the A-shared scan pair
    for BOTH passes (a matrix-pipe forward would leave the backward without its twin), a call that needs none takes dm_ssd_fwd."""
    from diffma_amd import selective_scan_interface as ssi

    L_ = _lib()
    log, real = [], L_.call
    monkeypatch.setattr(L_, "call", lambda name, a, st: (log.append(name), real(name, a, st))[1])
    Hm = 8                                               # rows of zxbcdt are 2 * 512 + 32 + 8 elements: 16-byte aligned, as the kernels need
    Din, L, Bsz = Hm * P, 200, 1
    Cx = Din + 2 * N
    g = torch.Generator().manual_seed(200)
    zx = (torch.randn(Bsz, L, 2 * Din + 2 * N + Hm, generator=g) * 0.5).to(BF16).to(gpu)
    conv_w, conv_b = (torch.randn(Cx, 4, generator=g) * 0.3).to(gpu), (torch.randn(Cx, generator=g) * 0.1).to(gpu)
    idx = torch.stack([torch.arange(L), torch.randperm(L, generator=g)]).int().to(gpu)
    inv = torch.argsort(idx.long(), dim=1).int()
    par = [A_H.float().repeat(2).to(gpu), D_H.float().repeat(2).to(gpu), BIAS_H.float().repeat(2).to(gpu), torch.ones(Din, device=gpu)]
    run = lambda zin: ssi.spiral_ssd(zin, conv_w, conv_b, par[2], par[0], par[1], par[3], 1e-5, idx, inv, Din, N)
    with torch.no_grad():
        y0 = run(zx)
    torch.cuda.synchronize()
    assert "dm_ssd_fwd" in log and "dm_selective_scan_fwd" not in log, log
    del log[:]
    zg = zx.clone().requires_grad_(True)
    y1 = run(zg)
    y1.backward(torch.ones_like(y1))
    torch.cuda.synchronize()
    assert "dm_selective_scan_fwd" in log and "dm_selective_scan_bwd" in log and not [n for n in log if n.startswith("dm_ssd")], log
    assert bool(torch.isfinite(zg.grad.float()).all())
    torch.testing.assert_close(y1.float(), y0.float(), rtol=3e-2, atol=5e-2 * max(1.0, float(y0.float().abs().max())))     # the TOL of test_kernels_gpu.py
