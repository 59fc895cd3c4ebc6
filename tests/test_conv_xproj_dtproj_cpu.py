"""The fused conv + x_proj kernels (csrc/conv_xproj.hip: K3x forward, K4x backward in its per-sequence, whole-sample and slab forms) and
the dt_proj kernels (csrc/dtproj.hip: K8, K8b): the parts that need no GPU.

Input builders, fp64 references, fp32 emulations that round where the kernels round, bound functions, `*_eval` functions and their
self-tests.  tests/test_conv_xproj_dtproj_gpu.py imports all of it and feeds the kernels' outputs to the same `*_eval` functions.
Symbols (u, T, F, EPS32, c(z), c'(z)) are those of tests/test_mixer_passes_cpu.py; the MFMA products take the bound of
tests/test_gemm_gpu.py: 2 Kc EPS32 S with S the fp64 product of the magnitudes.

Layer 1, exact cases (`mode="int"`).  Every product is linear apart from SiLU and softplus.  Operands are small integers; the fp64
reference asserts that every value stored in 16 bits is an integer of magnitude <= 256 (bf16) / 2048 (fp16) and that every fp32 sum
stays below 2^24 (`_assert_exact`), so the expected output is the fp64 result converted to the I/O dtype, bit for bit (the sign of a
zero apart: `exact`).
  * K3x and the per-sequence K4x run with silu = False.
  * The merged K4x forms are SiLU-only: conv bias 64 and |sum w x| <= 40 give pre >= 24, where silu'(pre) == 1.0f in fp32 for
    sigmoid_f (dm_common.h:316) and for the fast_exp2 / fast_rcp form of the slab kernel (conv_xproj.hip:660-663):
    exp2(-24 LOG2E) = 3.8e-11 < 2^-25, so 1 + e == 1.0f whatever the last bit of v_exp_f32, rcp(1) == 1, 1 + pre * 0 == 1
    (test_silu_prime_saturates_to_one).
  * K8: bias such that pre >= 21: softplus16_f returns x on its x > 20 branch (dtproj.hip:31).
  * `mode="seq"` (merged K4x only): the same integers with du up to 200 (fp16: 1500), so that the running sum of dx LEAVES the exact
    range of the I/O dtype.  Every fp32 value is still an exact integer; the expected result is the sequence of roundings the kernel
    documents (conv_xproj.hip:250-251, 467): sum_k = round(sum_{k-1} + dx_k) in direction order.  This is the one case that tells
    "rounded per direction" from "rounded once", which no bound can (fewer roundings are closer to fp64).

Layer 2, real values (`mode="real"`), per element against fp64 on the rounded inputs.
  * x~ (conv_xproj.hip:113-117): acc = bias, W products added one by one in fp32 (the compiler may contract them: fewer roundings),
    then silu_f, one rounding on the way out.  S_pre = |bias| + sum_k |w_k x_k|, E_pre = (W + 1) EPS32 S_pre;
        |x~ - ref| <= u |ref| + T + F + 1.1 E_pre + c(pre) |ref|           (|silu'| <= 1.1; silu = False: E_pre alone)
  * x_dbl (conv_xproj.hip:136-152): the reference is the fp64 product of the kernel's OWN rounded x~ with wx; two MFMA chains of
    D / 64 steps meet in one fp32 addition (red[], conv_xproj.hip:143-147):
        |x_dbl - ref| <= u |ref| + T + 2 (D + 1) EPS32 sum_d |x~ wx|
    Columns >= nproj of the x_dbl rows keep their sentinel.
  * g = (du + dx_dbl . Wx) silu'(pre) (conv_xproj.hip:377-411, 636-664): the K = 64 product plus one addition,
        E_g = 2 (64 + 1) EPS32 (|dx_dbl| . |Wx| + |du|) |silu'| + |du + dx_dbl . Wx| (c'(pre) m(pre) + E_pre / 2)
    with m(z) = sg (1 + |z| (1 - sg)) the magnitude form of silu' and |silu''| <= 1/2 carrying the error of pre.
  * dx per direction (conv_xproj.hip:416-418, 684-686): W products added in fp32 and one rounding,
        |dx - ref| <= u |ref| + T + F + sum_j |w_j| E_g[.] + (W + 1) EPS32 sum_j |w_j g[.]|
  * merged dx (conv_xproj.hip:425-431, 687-688): the running sum is rounded once per direction.  With P_k the reference's partial
    sums in direction order and e_k the fp32 terms of direction k above,
        |dx - ref| <= (1 + u)^ndir sum_k ((u + EPS32) |P_k| + e_k) + ndir T + F
  * dw / db (conv_xproj.hip:414-415, 667-668, 741-748): the partial rows are added in fp64 by the test; one fp32 accumulator takes
    `chain` rows (per-sequence: L; whole-sample: ndir L; slab: ndir L per sample of the workgroup, then 8 segments):
        |dw - ref| <= (chain + 4) EPS32 sum |g x| + sum E_g |x| + F,     db alike with x = 1.
  * delta (dtproj.hip:27-32, 91-97): pre = one K = 32 MFMA plus the bias, E = 2 (32 + 1) EPS32 (|x| . |w| + |bias|); softplus16_f
    has three branches and the bound takes the largest of those the fp64 pre +- E can reach:
        x > 20:       returns x; softplus(x) - x <= e^-20
        e < 2^-12:    returns e = exp2(x LOG2E): |e - log1p(e)| <= e^2 / 2 (2^-13 relative) + (2|x| + 4) EPS32 e
        otherwise:    log2(1 + e) LN2: the rounding of 1 + e is EPS32 (1 + e) on the argument, i.e. EPS32 ABSOLUTE on the logarithm
                      (this is what is left of the relative accuracy as e -> 2^-12), v_log_f32 another, the error of e enters as
                      (2|x| + 4) EPS32 e / (1 + e), and the two products cost 6 EPS32 |ref|
        |delta - ref| <= u |ref| + T + F + (E sigmoid(pre) + branch term) (1 + u)
  * K8b (dtproj.hip:251-321): dxdbl = 8 wave partials of dim / 256 MFMAs each, summed in LDS: u |ref| + T + 2 (dim + 8) EPS32 S;
    dW (partial images added in fp64): 2 (rows + 32) EPS32 S.  Columns >= rank of the dxdbl rows keep their sentinel.

The emulations use torch's accurate exp2 / log2 and a correctly rounded division for the 1-ulp hardware instructions.  Largest
error-to-bound ratio of the emulation over the cases of this file (test_emulation_meets_every_bound prints them):
    xproj_fwd        bf16 0.995  fp16 0.996
    xproj_bwd_seq    bf16 0.988  fp16 0.951        its dw / db (.dwdb)  bf16 0.013  fp16 0.024
    xproj_bwd_whole  bf16 0.966  fp16 0.924        its dw / db          bf16 0.013  fp16 0.012
    xproj_bwd_slab   bf16 0.980  fp16 0.944        its dw / db          bf16 0.008  fp16 0.008
    dtproj_fwd       bf16 0.994  fp16 0.989
    dtproj_bwd       bf16 0.861  fp16 0.474        its dW (.dW)         bf16 0.015  fp16 0.037
(16-bit outputs: nearly all of it is the output's own half-ulp rounding, charged as u |ref|.  The fp32 reductions are booked apart:
their bounds are worst-case sums of |term|, which random signs stay far below -- and a single missing row still exceeds them.)
"""
from types import SimpleNamespace as NS

import pytest
import torch

from tests.test_mixer_passes_cpu import (BF16, EPS32, F16, F32, FLOOR, LOG2E, NAME, NAN, TINY, UNIT, _fails, bits_equal, c_p,
                                         c_z, check, rnd, sig32, trunc)
from tests.test_mixer_passes_cpu import exact as _exact_bits

IO = [BF16, F16]
IO_IDS = [NAME[d] for d in IO]
INT_MAX = {BF16: 256, F16: 2048}
SENT = 7.0
NPROJ_B = 64                                # the projection width K4x is built for
LN2 = 0.6931471805599453
F64 = torch.float64

OPERATORS = ("xproj_fwd", "xproj_bwd_seq", "xproj_bwd_seq.dwdb", "xproj_bwd_whole", "xproj_bwd_whole.dwdb", "xproj_bwd_slab",
             "xproj_bwd_slab.dwdb", "dtproj_fwd", "dtproj_bwd", "dtproj_bwd.dW")       # .dwdb / .dW: the fp32 reductions, booked apart
RATIOS = {}                                 # (operator, dtype name) -> largest error / bound the GPU file has seen


def exact(op, dt, name, got, want, book=None):
    """Bit for bit, except the sign of a zero: a sum of products that comes out as zero is +0 or -0 after the order and the
    contraction of its terms (an accumulator that starts at +0.0f never returns -0), which no reference can foretell."""
    canon = lambda t: (t.detach().cpu().float() + 0.0).to(t.dtype)
    _exact_bits(op, dt, name, canon(got), canon(want), book)


def ints(g, shape, hi, p=1.0):
    """Integers in [-hi, hi], a share 1 - p of them zeroed."""
    v = torch.randint(-hi, hi + 1, shape, generator=g).double()
    if p < 1.0:
        v = v * (torch.rand(shape, generator=g, dtype=F64) < p)
    return v


def _assert_exact(dt, stored=(), sums=()):
    """The range conditions of an exact case: 16-bit values are integers inside the dtype's exact range, fp32 sums below 2^24."""
    for v in stored:
        assert bool((v == v.round()).all()) and float(v.abs().max()) <= INT_MAX[dt], f"16-bit value out of range: {float(v.abs().max())}"
    for v in sums:
        assert bool((v == v.round()).all()) and float(v.abs().max()) < 2 ** 24, f"fp32 sum out of range: {float(v.abs().max())}"


def _tables(g, L, ndir, table):
    if not table:
        return None
    return torch.stack([torch.arange(L)] + [torch.randperm(L, generator=g) for _ in range(ndir - 1)]).to(torch.int32) if ndir > 1 \
        else torch.randperm(L, generator=g).view(1, L).to(torch.int32)


def _gather(c, x):
    """[B, L, D] -> [ndir, B, L, D]: the rows of every direction in gathered order."""
    if c.idx is None:
        return x[None]
    return torch.stack([x[:, c.idx[k].long()] for k in range(c.ndir)])


def _windows(xs, W):
    """[.., L, D] -> [.., L, W, D]: tap k of row l is xs[l - (W - 1) + k], zero before the sequence."""
    L = xs.shape[-2]
    pad = torch.nn.functional.pad(xs, (0, 0, W - 1, 0))
    return torch.stack([pad[..., k:k + L, :] for k in range(W)], -2)


def _pre(c, win):
    """bias + sum_k w_k x_k in the kernel's order; fp64 or fp32 after the dtype of `win`."""
    w = c.w.to(win.dtype)
    acc = (c.bias.to(win.dtype) if c.bias is not None else torch.zeros(c.D, dtype=win.dtype)).expand(win.shape[:-2] + (c.D,)).clone()
    for k in range(c.W):
        acc = acc + w[:, k] * win[..., k, :]
    return acc


# =====================================================================================================================================
# K3x  dm_gather_conv1d_xproj_fwd
# =====================================================================================================================================
def xp_case(dt, B, L, D, P, W, ndir, table, w16, has_bias, mode, seed=0):
    """x [B, L, D], conv w [D, W] / bias [D] (fp32 or dt), wx [P, D], row tables [ndir, L].  mode "int": silu off, exact; "real": silu."""
    g = torch.Generator().manual_seed(seed)
    wdt = dt if w16 else F32
    if mode == "int":
        x = ints(g, (B, L, D), 2).to(dt)
        w = ints(g, (D, W), 2).to(wdt)
        bias = ints(g, (D,), 3).to(wdt) if has_bias else None
        wx = ints(g, (P, D), 1, p=min(0.75, 48.0 / D)).to(dt)
    else:
        x = torch.randn(B, L, D, generator=g, dtype=F64).to(dt)
        x[0, 0, :8] = torch.tensor([30.0, -30.0, 0.0, -0.0, 8.0, -8.0, 1e-3, -1.278]).to(dt)
        w = (0.5 * torch.randn(D, W, generator=g, dtype=F64)).to(wdt)
        bias = (0.3 * torch.randn(D, generator=g, dtype=F64)).to(wdt) if has_bias else None
        wx = (0.1 * torch.randn(P, D, generator=g, dtype=F64)).to(dt)
    return NS(dt=dt, B=B, L=L, D=D, P=P, W=W, ndir=ndir, silu=mode != "int", mode=mode, x=x, w=w, bias=bias, wx=wx,
              idx=_tables(g, L, ndir, table or ndir > 1), xd_sr=72)


def xp_emul(c, defect=None):
    """(x~ [ndir B, L, D], x_dbl frame [ndir B L, xd_sr]) as conv_xproj_fwd_kernel computes them."""
    st = trunc if defect == "truncate" else rnd
    win = _windows(_gather(c, c.x.float()), c.W)
    if defect == "halo16" and c.L > 16:                     # the window of row 16 starts from zeros again
        for k in range(c.W - 1):
            win[..., 16:16 + (c.W - 1 - k), k, :] = 0.0
    if defect == "drop_tap":
        win[..., 0, :] = 0.0
    acc = _pre(c, win)
    if c.silu:
        acc = acc * sig32(acc)
    xc = st(acc, c.dt)
    a = (acc if defect == "unrounded_a" else xc.float()).reshape(-1, c.D)
    wx = c.wx.float()
    h = c.D // 2
    prod = a[:, :h] @ wx[:, :h].t()
    if defect != "khalf":
        prod = prod + a[:, h:] @ wx[:, h:].t()
    frame = torch.full((a.shape[0], c.xd_sr), SENT, dtype=c.dt)
    frame[:, :c.P] = st(prod, c.dt)
    if defect == "alias_col":                               # the columns of the wave's last tile past nproj take column nproj - 1
        frame[:, c.P:-(-c.P // 16) * 16] = frame[:, c.P - 1:c.P]
    return xc.reshape(c.ndir * c.B, c.L, c.D), frame


def xp_eval(c, xc, xdbl, book=None, op="xproj_fwd"):
    u, T = UNIT[c.dt], TINY[c.dt]
    win = _windows(_gather(c, c.x.double()), c.W)
    pre = _pre(c, win)
    ref = (pre * torch.sigmoid(pre) if c.silu else pre).reshape(c.ndir * c.B, c.L, c.D)
    xdbl = xdbl.detach().cpu()
    assert tuple(xdbl.shape) == (c.ndir * c.B * c.L, c.xd_sr)
    assert bool((xdbl[:, c.P:].float() == SENT).all()), f"{op}: columns >= nproj of the x_dbl rows were written"
    wx = c.wx.double()
    if c.mode == "int":
        rdbl = ref.reshape(-1, c.D) @ wx.t()
        _assert_exact(c.dt, stored=(ref, rdbl), sums=(ref.reshape(-1, c.D).abs() @ wx.abs().t(),))
        exact(op, c.dt, "x~", xc, ref.to(c.dt), book)
        exact(op, c.dt, "x_dbl", xdbl[:, :c.P], rdbl.to(c.dt), book)
        return 0.0
    S = _pre(NS(w=c.w.double().abs(), bias=None if c.bias is None else c.bias.double().abs(), D=c.D, W=c.W), win.abs())
    Epre = ((c.W + 1) * EPS32 * S).reshape(ref.shape)
    pre = pre.reshape(ref.shape)
    tol = u * ref.abs() + T + FLOOR + (1.1 * Epre + c_z(pre) * ref.abs() if c.silu else Epre)
    r = check(op, c.dt, "x~", xc, ref, tol, book)
    a = xc.detach().cpu().double().reshape(-1, c.D)
    rdbl = a @ wx.t()
    tol = u * rdbl.abs() + T + 2 * (c.D + 1) * EPS32 * (a.abs() @ wx.abs().t())
    return max(r, check(op, c.dt, "x_dbl", xdbl[:, :c.P], rdbl, tol, book))


# (B, L, D, P, W, ndir, table at ndir 1, 16-bit conv weights, bias): sequence lengths 1 .. 49 (a window shorter than W, the carry across
# one and two tile boundaries, ragged last tiles), nproj with whole waves off and partial last column tiles, every width and dim
XP_SHAPES = [(2, 1, 128, 1, 4, 1, False, False, True), (1, 2, 256, 15, 3, 3, True, True, True), (1, 3, 1024, 16, 2, 1, True, False, False),
             (2, 15, 128, 17, 4, 3, True, True, False), (1, 16, 256, 33, 2, 3, True, False, True),
             (2, 17, 128, 48, 3, 3, True, False, True), (1, 17, 1024, 49, 4, 3, True, True, True),
             (1, 31, 128, 64, 2, 1, False, True, False), (1, 32, 512, 64, 4, 3, True, False, True),
             (2, 33, 256, 49, 4, 3, True, False, False), (1, 33, 128, 33, 3, 1, True, True, True),
             (1, 33, 1024, 15, 2, 3, True, False, True), (1, 49, 128, 64, 4, 3, True, False, True),
             (1, 49, 1024, 17, 3, 1, False, True, False), (1, 49, 256, 1, 2, 3, True, False, True),
             (1, 17, 128, 16, 2, 1, False, False, True)]
XP_IDS = ["B%d-L%d-D%d-P%d-W%d-nd%d-t%d-w16_%d-b%d" % tuple(int(v) for v in s) for s in XP_SHAPES]


def xp_cases(dt, mode):
    return [xp_case(dt, *s, mode, seed=1000 + i) for i, s in enumerate(XP_SHAPES)]


# =====================================================================================================================================
# K4x  dm_gather_conv1d_xproj_bwd: per-sequence ("seq"), whole-sample merged ("whole") and slab merged ("slab") forms
# =====================================================================================================================================
def xb_case(dt, form, B, L, D, W, ndir, table, w16, has_bias, mode, seed=0):
    """x [B, L, D], conv w / bias, wxt [D, 64], du [ndir B, L, D], dxdbl [ndir B L, 64], row tables.  The merged forms ("whole", "slab")
    are SiLU-only: their exact modes saturate silu' with bias 64."""
    g = torch.Generator().manual_seed(seed)
    wdt = dt if w16 else F32
    merged = form != "seq"
    S = ndir * B
    if mode == "real":
        x = torch.randn(B, L, D, generator=g, dtype=F64).to(dt)
        w = (0.5 * torch.randn(D, W, generator=g, dtype=F64)).to(wdt)
        bias = (0.3 * torch.randn(D, generator=g, dtype=F64)).to(wdt) if has_bias else None
        wxt = (0.1 * torch.randn(D, NPROJ_B, generator=g, dtype=F64)).to(dt)
        du = torch.randn(S, L, D, generator=g, dtype=F64).to(dt)
        dxdbl = torch.randn(S * L, NPROJ_B, generator=g, dtype=F64).to(dt)
    else:
        x = ints(g, (B, L, D), 3).to(dt)
        w = ints(g, (D, W), 2).to(wdt)
        bias = (torch.full((D,), 64.0, dtype=F64) if merged else ints(g, (D,), 3)).to(wdt) if (has_bias or merged) else None
        wxt = ints(g, (D, NPROJ_B), 1, p=0.5).to(dt)
        du = ints(g, (S, L, D), (200 if dt == BF16 else 1500) if mode == "seq" else 3).to(dt)
        dxdbl = ints(g, (S * L, NPROJ_B), 2, p=0.5).to(dt)
    return NS(dt=dt, form=form, merged=merged, B=B, L=L, D=D, W=W, ndir=ndir, silu=merged or mode == "real", mode=mode, x=x, w=w,
              bias=bias, wxt=wxt, du=du, dxdbl=dxdbl, idx=_tables(g, L, ndir, table or ndir > 1 or merged))


def _to_token(c, dxg):
    """[ndir, B, L, D] in gathered order -> token order."""
    if c.idx is None:
        return dxg
    out = torch.zeros_like(dxg)
    for k in range(c.ndir):
        out[k][:, c.idx[k].long()] = dxg[k]
    return out


def _conv_t(c, g, w):
    """dx[l] = w[W-1] g[l] + sum_k w[W-2-k] g[l+1+k] in the kernel's order (rows past the sequence are zero); g [.., L, D]."""
    W, L = c.W, c.L
    pad = torch.nn.functional.pad(g, (0, 0, 0, W - 1))
    acc = w[:, W - 1] * g
    for k in range(W - 1):
        acc = acc + w[:, W - 2 - k] * pad[..., 1 + k:1 + k + L, :]
    return acc


def xb_emul(c, defect=None):
    """(dx, dw partial rows [rows, D, W], db partial rows [rows, D]); dx is [ndir B, L, D] per direction or the merged [B, L, D]."""
    st = trunc if defect == "truncate" else rnd
    nd, B, L, D, W = c.ndir, c.B, c.L, c.D, c.W
    win = _windows(_gather(c, c.x.float()), W)
    w = c.w.float()
    g = c.dxdbl.float().view(nd, B, L, NPROJ_B) @ c.wxt.float().t() + c.du.float().view(nd, B, L, D)
    if c.silu:
        pre = _pre(NS(w=c.w, bias=None if defect == "no_bias_in_pre" else c.bias, D=D, W=W), win)
        sg = sig32(pre)
        g = g * (sg * (1.0 + pre * (1.0 - sg)))
    gx = g
    if defect == "ragged_pad":                              # the rows after the sequence repeat the gradient of row L - 1
        gx = torch.cat([g, g[..., L - 1:, :].expand(nd, B, W - 1, D)], -2)
        dxg = _conv_t(NS(W=W, L=L + W - 1), gx, w)[..., :L, :]
    else:
        dxg = _conv_t(c, g, w)
    tok = dxg.clone() if defect == "dx_gathered_row" else None
    dxt = _to_token(c, dxg)
    if tok is not None:
        dxt[nd - 1] = tok[nd - 1]
    if c.merged:
        if defect == "sum_once":
            dx = st(dxt.sum(0), c.dt)
        else:
            dx = torch.zeros(B, L, D, dtype=c.dt)
            for k in range(nd):
                dx = st(dx.float() + dxt[k], c.dt)
    else:
        dx = st(dxt, c.dt).reshape(nd * B, L, D)
    dw = torch.zeros(nd, B, D, W, dtype=F32)
    db = torch.zeros(nd, B, D, dtype=F32)
    seg = -(-L // 8)
    for l in range(L - 1, -1, -1):
        gl = g[:, :, l].clone()
        if defect == "dw_miss_row" and l == L // 2:
            gl[nd - 1, 0] = 0.0
        if defect == "halo_owned" and l == min(seg, L - 1):
            gl[0] = 2 * gl[0]
        dw = dw + gl[..., None] * win[:, :, l].transpose(-1, -2)
        db = db + gl
    if c.merged:
        dwp, dbp = dw[0], db[0]
        for k in range(1, nd):
            dwp, dbp = dwp + dw[k], dbp + db[k]
        return dx, dwp, dbp
    return dx, dw.reshape(nd * B, D, W), db.reshape(nd * B, D)


def xb_chain(c, rows_with_sums=None):
    """Rows one fp32 accumulator of dw / db takes (the bound's `chain`)."""
    if c.form == "seq":
        return c.L
    if c.form == "whole" or not rows_with_sums:
        return c.ndir * c.L
    return c.ndir * c.L * -(-c.B // rows_with_sums) + 8


def xb_eval(c, dx, dwp, dbp, chain=None, book=None, op=None):
    """dx against fp64 (bitwise in the exact modes); the partial rows of dw / db are added in fp64 first."""
    op = op or "xproj_bwd_" + c.form
    u, T = UNIT[c.dt], TINY[c.dt]
    nd, B, L, D, W = c.ndir, c.B, c.L, c.D, c.W
    chain = chain or xb_chain(c)
    win = _windows(_gather(c, c.x.double()), W)
    w = c.w.double()
    p = c.dxdbl.double().view(nd, B, L, NPROJ_B) @ c.wxt.double().t()
    du = c.du.double().view(nd, B, L, D)
    gs = p + du
    Sp = c.dxdbl.double().abs().view(nd, B, L, NPROJ_B) @ c.wxt.double().abs().t() + du.abs()
    if c.silu:
        pre = _pre(c, win)
        sg = torch.sigmoid(pre)
        fac = sg * (1 + pre * (1 - sg))
    g = gs * fac if c.silu else gs
    dxg = _conv_t(c, g, w)
    dxt = _to_token(c, dxg)
    dwr = torch.einsum("sbld,sblkd->dk", g, win)
    dbr = g.sum((0, 1, 2))
    dw = dwp.detach().cpu().double().reshape(-1, D, W).sum(0)
    db = dbr.clone() if dbp is None else dbp.detach().cpu().double().reshape(-1, D).sum(0)     # db_partial == NULL: no such output
    dx = dx.detach().cpu()
    if c.mode != "real":
        if c.silu:                                          # the saturation the exact merged cases stand on
            assert float(pre.min()) >= 24.0 and float((pre - 64.0).abs().max()) <= 40.0
        _assert_exact(c.dt, sums=(Sp, _conv_t(c, gs.abs(), w.abs()), torch.einsum("sbld,sblkd->dk", gs.abs(), win.abs()),
                                  gs.abs().sum((0, 1, 2))))
        if c.merged:
            run = torch.zeros(B, L, D, dtype=F64)
            for k in range(nd):
                if c.mode == "int":
                    _assert_exact(c.dt, stored=(run + dxt[k],))
                run = (run + dxt[k]).to(c.dt).double()
            if c.mode == "seq" and nd > 1:
                assert float(dxt.sum(0).abs().max()) > INT_MAX[c.dt] and not bits_equal(dxt.sum(0).to(c.dt), run.to(c.dt))
            want = run.to(c.dt)
        else:
            _assert_exact(c.dt, stored=(dxt,))
            want = dxt.to(c.dt).reshape(nd * B, L, D)
        exact(op, c.dt, "dx", dx, want, book)
        exact(op + ".dwdb", c.dt, "dw", dw.float(), dwr.float(), book)
        exact(op + ".dwdb", c.dt, "db", db.float(), dbr.float(), book)
        return 0.0
    Eg = 2 * (NPROJ_B + 1) * EPS32 * Sp
    if c.silu:
        Spre = _pre(NS(w=w.abs(), bias=None if c.bias is None else c.bias.double().abs(), D=D, W=W), win.abs())
        Eg = Eg * fac.abs() + gs.abs() * (c_p(pre) * sg * (1 + pre.abs() * (1 - sg)) + 0.5 * (W + 1) * EPS32 * Spre)
    e = _to_token(c, _conv_t(c, Eg, w.abs()) + (W + 1) * EPS32 * _conv_t(c, g.abs(), w.abs()))
    if c.merged:
        ref = dxt.sum(0)
        part = torch.cumsum(dxt, 0).abs()
        tol = (1 + u) ** nd * ((u + EPS32) * part + e).sum(0) + nd * T + FLOOR
    else:
        ref = dxt.reshape(nd * B, L, D)
        tol = (u * dxt.abs() + T + FLOOR + e).reshape(ref.shape)
    r = check(op, c.dt, "dx", dx, ref, tol, book)
    tw = (chain + 4) * EPS32 * torch.einsum("sbld,sblkd->dk", g.abs(), win.abs()) + torch.einsum("sbld,sblkd->dk", Eg, win.abs()) + FLOOR
    r = max(r, check(op + ".dwdb", c.dt, "dw", dw, dwr, tw, book))
    tb = (chain + 4) * EPS32 * g.abs().sum((0, 1, 2)) + Eg.sum((0, 1, 2)) + FLOOR
    return max(r, check(op + ".dwdb", c.dt, "db", db, dbr, tb, book))


# per-sequence form: (B, L, D, W, ndir, table at ndir 1, 16-bit conv weights, bias)
XB_SEQ_SHAPES = [(2, 1, 128, 4, 1, False, False, True), (1, 2, 256, 3, 3, True, True, True), (1, 3, 1024, 2, 1, True, False, False),
                 (2, 15, 128, 4, 3, True, True, False), (1, 16, 256, 2, 3, True, False, True), (2, 17, 128, 3, 3, True, False, True),
                 (1, 17, 1024, 4, 3, True, True, True), (1, 31, 128, 2, 1, False, True, False), (1, 32, 512, 4, 3, True, False, True),
                 (2, 33, 256, 4, 3, True, False, False), (1, 33, 128, 3, 1, True, True, True), (1, 49, 128, 4, 3, True, False, True),
                 (1, 49, 1024, 3, 1, False, True, False), (1, 49, 256, 2, 3, True, False, True)]
# merged forms: (B, L, D, ndir, 16-bit conv weights).  Whole-sample form (DM_K4X_SLAB=0): the tiled lengths
XB_WHOLE_SHAPES = [(1, 1, 128, 1, False), (1, 2, 128, 3, True), (1, 3, 256, 3, False), (2, 15, 256, 4, False), (1, 16, 128, 3, True),
                   (1, 17, 1024, 3, False), (1, 31, 128, 1, False), (1, 32, 256, 3, True), (2, 33, 128, 4, False), (1, 49, 128, 3, False)]
# slab form (DM_K4X_SLAB=1): waves with empty segments (5, 8, 9), the default threshold (32, 33), the tile height flip (100, 104: 16-row
# tiles, 105: 14-row), the model's 196, token 255 in the uint8_t table
XB_SLAB_SHAPES = [(1, 5, 128, 3, False), (2, 8, 256, 1, True), (1, 9, 128, 4, False), (2, 32, 128, 3, False), (1, 33, 256, 4, True),
                  (1, 100, 128, 3, False), (1, 104, 128, 1, False), (1, 105, 256, 3, True), (1, 196, 128, 3, False),
                  (1, 196, 1024, 3, False), (1, 255, 128, 4, True), (2, 256, 256, 3, False)]
XB_THRESHOLD_L = [31, 32, 33]              # DM_K4X_SLAB unset: the library's own choice at its threshold


def _ids(shapes):
    return ["-".join(str(int(v)) for v in s) for s in shapes]


def xb_seq_cases(dt, mode):
    return [xb_case(dt, "seq", *s, mode, seed=2000 + i) for i, s in enumerate(XB_SEQ_SHAPES)]


def xb_merged_case(dt, form, shape, mode, seed):
    B, L, D, nd, w16 = shape
    return xb_case(dt, form, B, L, D, 4, nd, True, w16, True, mode, seed=seed)


def xb_merged_cases(dt, form, mode):
    shapes = XB_WHOLE_SHAPES if form == "whole" else XB_SLAB_SHAPES
    return [xb_merged_case(dt, form, s, mode, 3000 + i) for i, s in enumerate(shapes)]


# =====================================================================================================================================
# K8  dm_dtproj_softplus_fwd
# =====================================================================================================================================
def dt_case(dt, M, Dm, R, has_bias, mode, seed=0):
    """xdbl [M, xd_sr] with NaN in the columns >= R (they must not be read), w [Dm, R], bias [Dm] fp32.  mode "int": pre >= 21;
    "real": pre over the three branches of the softplus; "band": pre dense in [-9, -4] (e between 2^-13 and 2^-6)."""
    g = torch.Generator().manual_seed(seed)
    xd_sr = 40 if R < 32 else 48
    xd = torch.full((M, xd_sr), NAN, dtype=dt)
    if mode == "int":
        xd[:, :R] = ints(g, (M, R), 2).to(dt)
        w = ints(g, (Dm, R), 1).to(dt)
        bias = (64.0 + ints(g, (Dm,), 6)).float()
        has_bias = True
    elif mode == "band":
        xd[:, :R] = (0.05 * torch.randn(M, R, generator=g, dtype=F64)).to(dt)
        w = (0.2 * torch.randn(Dm, R, generator=g, dtype=F64)).to(dt)
        bias = torch.linspace(-9.0, -4.0, Dm).float()
        has_bias = True
    else:
        xd[:, :R] = torch.randn(M, R, generator=g, dtype=F64).to(dt)
        w = (torch.randn(Dm, R, generator=g, dtype=F64) * 10.0 ** (1.5 * torch.rand(Dm, 1, generator=g, dtype=F64) - 1)).to(dt)
        bias = (4 * torch.randn(Dm, generator=g)).float()
        bias[:4] = torch.tensor([20.0, -8.3178, 25.0, -20.0])[:Dm]              # around both branch points and far into each tail
    return NS(dt=dt, M=M, Dm=Dm, R=R, xd_sr=xd_sr, xdbl=xd, w=w, bias=bias if has_bias else None, mode=mode)


def dt_emul(c, defect=None):
    st = trunc if defect == "truncate" else rnd
    R = c.R
    if defect == "rank_mask":                               # one more lane group of 8 reduction elements on each side
        R = c.R + 8 if c.R < 32 else c.R - 8
        x = c.xdbl[:, :R].float()
        w = torch.cat([c.w.float(), torch.ones(c.Dm, 8)], 1)[:, :R]
    else:
        x, w = c.xdbl[:, :R].float(), c.w.float()
    pre = x @ w.t()
    if c.bias is not None:
        pre = pre + c.bias
    e = torch.exp2(pre * torch.tensor(LOG2E, dtype=F32))
    big = torch.log2(1.0 + e) * torch.tensor(LN2, dtype=F32)
    r = torch.where(e < (2.0 ** -8 if defect == "small_e_2^-8" else 2.0 ** -12), e, big)
    return st(torch.where(pre > 20.0, pre, r), c.dt)


def dt_eval(c, delta, book=None, op="dtproj_fwd"):
    u, T = UNIT[c.dt], TINY[c.dt]
    x, w = c.xdbl[:, :c.R].double(), c.w.double()
    b = c.bias.double() if c.bias is not None else torch.zeros(c.Dm, dtype=F64)
    pre = x @ w.t() + b
    if c.mode == "int":
        assert float(pre.min()) >= 21.0
        _assert_exact(c.dt, stored=(pre,), sums=(x.abs() @ w.abs().t() + b.abs(),))
        exact(op, c.dt, "delta", delta, pre.to(c.dt), book)
        return 0.0
    E = 2 * (32 + 1) * EPS32 * (x.abs() @ w.abs().t() + b.abs())
    ref = torch.nn.functional.softplus(pre, threshold=1e9)
    ref = torch.where(pre > 30, pre + torch.exp(-pre), ref)
    e = torch.exp(pre)
    rel = (2 * (pre.abs() + E) + 4) * EPS32
    grow = torch.exp(E)                                     # e at pre + E
    can_id, can_low = pre + E >= 20.0, pre - E <= 20.0
    zero = torch.zeros_like(pre)
    tA = torch.where(can_id, (pre - ref).abs(), zero)
    tB = torch.where(can_low & (e / grow * (1 - rel) < 2.0 ** -12), (e - ref).abs() + rel * e, zero)
    tC = torch.where(can_low & (e * grow * (1 + rel) >= 2.0 ** -12), 2 * EPS32 + rel * e / (1 + e) + 6 * EPS32 * ref, zero)
    branch = torch.maximum(tA, torch.maximum(tB, tC))
    tol = u * ref.abs() + T + FLOOR + (E * torch.sigmoid(pre) + branch) * (1 + u)
    return check(op, c.dt, "delta", delta, ref, tol, book)


DT_DIMS = [16, 64, 208, 256, 272, 1536]    # across the 64-column wave and the 256-column workgroup edges
DT_RANKS = [8, 16, 24, 32]
DT_ROWS = [1, 5, 16, 17, 33, 130]          # row tails of the 16-row tile; 130 rows: several tiles per workgroup
# (the last shape: 171 row tiles x 6 column blocks keep TWO tiles per workgroup in run_dtproj_fwd -- the prefetching tile loop and its
# early exit in the last workgroup; fewer rows are spread one tile per workgroup)
DT_SHAPES = [(DT_ROWS[(i + j) % 6], Dm, R) for i, Dm in enumerate(DT_DIMS) for j, R in enumerate(DT_RANKS)] + [(2725, 1536, 32)]


def dt_cases(dt, mode):
    return [dt_case(dt, M, Dm, R, (i % 5) != 0, mode, seed=4000 + i) for i, (M, Dm, R) in enumerate(DT_SHAPES)]


# =====================================================================================================================================
# K8b  dm_dtproj_bwd
# =====================================================================================================================================
def db_case(dt, M, Dm, R, mode, seed=0):
    """ddelta [M, Dm], xdbl [M, 40 | 48] (NaN past the rank), w [Dm, R]; dxdbl rows have stride 64 and a sentinel past the rank."""
    g = torch.Generator().manual_seed(seed)
    xd_sr = 40 if R < 32 else 48
    xd = torch.full((M, xd_sr), NAN, dtype=dt)
    if mode == "int":
        dd = ints(g, (M, Dm), 2, p=64.0 / Dm).to(dt)
        xd[:, :R] = ints(g, (M, R), 3).to(dt)
        w = ints(g, (Dm, R), 2).to(dt)
    else:
        dd = torch.randn(M, Dm, generator=g, dtype=F64).to(dt)
        xd[:, :R] = torch.randn(M, R, generator=g, dtype=F64).to(dt)
        w = (0.1 * torch.randn(Dm, R, generator=g, dtype=F64)).to(dt)
    return NS(dt=dt, M=M, Dm=Dm, R=R, xd_sr=xd_sr, dxd_sr=64, dd=dd, xdbl=xd, w=w, mode=mode)


def db_nblks(M):
    """nblk values of a case: 1, 2 and ceil(rows / 32) where legal (2 does not divide 3 tiles: workgroups own 2 and 1 tiles)."""
    nt = -(-M // 32)
    return sorted({1, min(2, nt), nt})


def db_emul(c, nblk, defect=None):
    """(dxdbl frame [M, 64], part [nblk, Dm, R]) as dtproj_bwd_kernel computes them."""
    st = trunc if defect == "truncate" else rnd
    dd, x, w = c.dd.float(), c.xdbl[:, :c.R].float(), c.w.float()
    CH = c.Dm // 8
    s = torch.zeros(c.M, c.R, dtype=F32)
    for wv in range(8):
        s = s + dd[:, wv * CH:(wv + 1) * CH] @ w[wv * CH:(wv + 1) * CH]
    frame = torch.full((c.M, c.dxd_sr), SENT, dtype=c.dt)
    frame[:, :c.R] = st(s, c.dt)
    part = torch.zeros(nblk, c.Dm, c.R, dtype=F32)
    nt = -(-c.M // 32)
    for t in range(nt):
        rows = slice(32 * t, min(32 * t + 32, c.M))
        part[t % nblk] = part[t % nblk] + dd[rows].t() @ x[rows]
        if defect == "row_twice" and t == nt - 1 and c.M % 32:
            part[t % nblk] = part[t % nblk] + dd[c.M - 1:].t() @ x[c.M - 1:]
    return frame, part


def db_eval(c, dxdbl, part, book=None, op="dtproj_bwd"):
    u, T = UNIT[c.dt], TINY[c.dt]
    dd, x, w = c.dd.double(), c.xdbl[:, :c.R].double(), c.w.double()
    dxdbl = dxdbl.detach().cpu()
    assert tuple(dxdbl.shape) == (c.M, c.dxd_sr)
    assert bool((dxdbl[:, c.R:].float() == SENT).all()), f"{op}: columns >= rank of the dxdbl rows were written"
    rx, rw = dd @ w, dd.t() @ x
    Sx, Sw = dd.abs() @ w.abs(), dd.abs().t() @ x.abs()
    dW = part.detach().cpu().double().reshape(-1, c.Dm, c.R).sum(0)
    if c.mode == "int":
        _assert_exact(c.dt, stored=(rx,), sums=(Sx, Sw))
        exact(op, c.dt, "dxdbl", dxdbl[:, :c.R], rx.to(c.dt), book)
        exact(op + ".dW", c.dt, "dW", dW.float(), rw.float(), book)
        return 0.0
    r = check(op, c.dt, "dxdbl", dxdbl[:, :c.R], rx, u * rx.abs() + T + 2 * (c.Dm + 8) * EPS32 * Sx, book)
    return max(r, check(op + ".dW", c.dt, "dW", dW, rw, 2 * (c.M + 32) * EPS32 * Sw + FLOOR, book))


DB_ROWS = [1, 5, 31, 32, 33, 64, 95]
DB_INST = [(512, 16), (512, 32), (768, 16), (768, 32), (1024, 16), (1024, 32)]
DB_SHAPES = [(DB_ROWS[(i + j) % 7], Dm, R) for i, (Dm, R) in enumerate(DB_INST) for j in range(3)] + [(M, 512, 16) for M in DB_ROWS[3:]]


def db_cases(dt, mode):
    return [db_case(dt, M, Dm, R, mode, seed=5000 + i) for i, (M, Dm, R) in enumerate(DB_SHAPES)]


# =====================================================================================================================================
# self-tests
# =====================================================================================================================================
def test_silu_prime_saturates_to_one():
    """pre >= 24 (bias 64, |sum w x| <= 40): silu'(pre) is exactly 1.0f for sigmoid_f and for the slab kernel's exp2 / rcp form, with
    room for the 1-ulp hardware instructions: e stays below 2^-25, where 1 + e rounds to 1."""
    pre = torch.cat([torch.arange(24, 105, dtype=F32), torch.linspace(24.0, 104.0, 4001)])
    sg = sig32(pre)
    assert bool((sg * (1.0 + pre * (1.0 - sg)) == 1.0).all())
    ex = pre * torch.tensor(-LOG2E, dtype=F32)                                  # conv_xproj.hip:660-663
    e = torch.exp2(ex)
    assert float(e.max()) * (1 + 2.0 ** -20) < 2.0 ** -25
    sg = 1.0 / (e + 1.0)
    assert bool((sg * (1.0 + pre * (1.0 - sg)) == 1.0).all())
    assert bool(((1.0 + torch.tensor([2.0 ** -25 * (1 - 2.0 ** -20)], dtype=F32)) == 1.0).all())


def xb_all_cases(dt, mode):
    """The K4x cases of one mode in its three forms; the exact mode brings the rounding-sequence cases of the merged forms along."""
    cs = xb_seq_cases(dt, mode)
    for form, shapes in (("whole", XB_WHOLE_SHAPES), ("slab", XB_SLAB_SHAPES)):
        cs += xb_merged_cases(dt, form, mode)
        if mode == "int":
            cs += [xb_merged_case(dt, form, s, "seq", 3500 + i) for i, s in enumerate(shapes)]
    return cs


def _emulate_all(book, mode):
    """Every case of the GPU file through its emulation and evaluation; returns the number of cases."""
    n = 0
    for dt in IO:
        for c in xp_cases(dt, mode):
            xp_eval(c, *xp_emul(c), book=book)
            n += 1
        for c in xb_all_cases(dt, mode):
            xb_eval(c, *xb_emul(c), book=book)
            n += 1
        for c in dt_cases(dt, mode) + (dt_cases(dt, "band") if mode == "real" else []):
            dt_eval(c, dt_emul(c), book=book)
            n += 1
        for c in db_cases(dt, mode):
            for nblk in db_nblks(c.M):
                db_eval(c, *db_emul(c, nblk), book=book)
                n += 1
    return n


def test_every_exact_case_is_in_range_and_exact():
    """Layer 1: the range asserts of every exact case hold on the fp64 reference, and the fp32 emulation reproduces it bit for bit."""
    assert _emulate_all({}, "int") > 0


def test_emulation_meets_every_bound():
    """Layer 2: the fp32 emulation of each operator, rounding where the kernel rounds, is inside every bound on every case."""
    book = {}
    _emulate_all(book, "real")
    for k in sorted(book):
        print(f"emulation {k[0]:20s} {k[1]}: {book[k]:.3f}")
    assert all(v < 1.0 for v in book.values())
    assert set(book) == {(op, NAME[dt]) for dt in IO for op in OPERATORS}


DEFECTS = {
    # name: (operator family, the emulation's defect switch)
    "window not carried across a tile boundary": ("xp", "halo16"),
    "last tap dropped": ("xp", "drop_tap"),
    "upper K-half of x_dbl lost": ("xp", "khalf"),
    "column >= nproj aliased onto column nproj-1": ("xp", "alias_col"),
    "x_dbl from the unrounded x~": ("xp", "unrounded_a"),
    "x~ truncated instead of rounded": ("xp", "truncate"),
    "padding rows of a ragged tile not zeroed": ("xb", "ragged_pad"),
    "one row missing from dw / db": ("xb", "dw_miss_row"),
    "a halo row counted as owned": ("xb", "halo_owned"),
    "dx added to the gathered row instead of the token row": ("xb", "dx_gathered_row"),
    "running sum rounded once instead of per direction": ("xb", "sum_once"),
    "conv bias missing from pre in silu'": ("xb", "no_bias_in_pre"),
    "dx truncated instead of rounded": ("xb", "truncate"),
    "rank mask off by one lane group": ("dt", "rank_mask"),
    "softplus small-e branch taken at 2^-8": ("dt", "small_e_2^-8"),
    "delta truncated instead of rounded": ("dt", "truncate"),
    "row rows-1 counted twice in dW": ("db", "row_twice"),
    "dxdbl truncated instead of rounded": ("db", "truncate"),
}


@pytest.mark.parametrize("name", list(DEFECTS))
def test_bounds_tell_each_defect_from_the_reference(name):
    """Each seeded defect, a variant of the emulation, is rejected by the layer-1 or the layer-2 evaluation on at least one of the
    cases the GPU file runs (the clean emulation passes all of them: the two tests above)."""
    fam, defect = DEFECTS[name]
    hit = 0
    for dt in IO:
        if fam == "xp":
            for mode in ("int", "real"):
                hit += sum(_fails(lambda: xp_eval(c, *xp_emul(c, defect), book={})) for c in xp_cases(dt, mode))
        elif fam == "xb":
            cs = [c for mode in ("int", "real") for c in xb_all_cases(dt, mode)[::2]]
            hit += sum(_fails(lambda: xb_eval(c, *xb_emul(c, defect), book={})) for c in cs)
        elif fam == "dt":
            for mode in ("int", "real", "band"):
                hit += sum(_fails(lambda: dt_eval(c, dt_emul(c, defect), book={})) for c in dt_cases(dt, mode)[::2])
        else:
            for mode in ("int", "real"):
                hit += sum(_fails(lambda: db_eval(c, *db_emul(c, db_nblks(c.M)[-1], defect), book={})) for c in db_cases(dt, mode))
    assert hit > 0, f"no case separates the defect '{name}' from the reference"
