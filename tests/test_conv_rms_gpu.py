"""K3 / K4 (csrc/conv.hip: dm_gather_conv1d_fwd / _bwd) and K9 (csrc/rmsnorm.hip: dm_rmsnorm_merge_fwd / _bwd) against fp64.

Most cases go through the C ABI with hand-built argument structs, so strides, view offsets, dtypes, part_ss and nchunk are chosen by
the test.  Inputs are rounded to their storage dtype first; the reference is plain torch fp64 (oracle.mamba_ref.causal_conv1d_ref on
the gathered sequences, the closed RMSNorm formula) with fp64 autograd for every gradient.  Every output and gradient is compared
per element; output buffers start as NaN (an element never written fails) and, where a row stride exceeds the width, the padding
holds a sentinel that must survive.

Bounds.  u = unit roundoff of the STORED dtype (2^-8 bf16, 2^-11 fp16, 0 fp32), TINY = 2^-24 absolute for fp16 subnormals,
EPS32 = 2^-24; the kernels compute in fp32, and one hardware transcendental (v_exp_f32, v_rcp_f32, v_rsq_f32) is good to
1 ulp = 2 EPS32.  Every bound scales with the sum of the magnitudes of the terms, not with |ref|.  None is taken from a measured error.

K3 forward.  pre = b + sum_k w_k x_k is W products and W additions, each rounded (or fused): |pre - ref| <= (W + 1) EPS32 P with
  P = |b| + sum_k |w_k x_k|; E_pre = (W + 2) EPS32 P leaves 1 / (W + 1) of slack, which also pays for the final rounding to the
  stored dtype being applied to the computed value instead of the reference (u E_pre).
  silu(pre) = pre * rcp(1 + exp2(-pre * LOG2E)): the exp2 argument carries two roundings (the product and the constant), i.e. an
  absolute error 2 |pre| LOG2E EPS32, which is a relative error 2 |pre| EPS32 of the power; v_exp_f32 adds 2 EPS32; the power
  enters 1 + e with the weight e / (1 + e) <= 1; the addition adds EPS32, v_rcp_f32 2 EPS32 and the product with pre EPS32:
  (2 |pre| + 2) + 1 + 2 + 1 = 6 + 2 |pre| <= C_SILU (1 + |pre|) with C_SILU = 8.  With |silu'| <= 1.1:
      |out - ref| <= u |ref| + TINY + 1.1 E_pre + C_SILU (1 + |pre|) EPS32 |ref|        (without SiLU: u |ref| + TINY + E_pre).
K4 dx.  g = dout * silu'(pre), silu' = sg h, h = 1 + pre q, q = 1 - sg, |silu''| <= 0.5.  With r = (2 |pre| + 2) q + 3 (the relative
  error of sg in EPS32, as counted above): d(sg) <= sg r, d(q) <= sg r + q, d(h) <= |pre| d(q) + |pre| q + |h|,
  d(sg h) <= |h| sg r + sg d(h) + sg |h|.  Using sg |h| = |silu'| <= 1.1, |pre| q sg <= 0.28, and |pre| sg^2 <= |pre| (pre > 0) or
  <= 0.14 (pre < 0):  1.1 (5 + 2 |pre|) + (0.7 + 3.56 |pre|) + 0.56 + 1.1 + 1.1 = 8.96 + 5.76 |pre|, plus 1.1 for the product
  with dout: <= C_DSILU (1 + |pre|) with C_DSILU = 11 (absolute, in units of |dout| EPS32).  So
      E_g = |dout| (0.5 E_pre + C_DSILU (1 + |pre|) EPS32)            (0 without SiLU: g = dout exactly),
      |dx - ref| <= u |ref| + TINY + sum_j |w_j| E_g_j + (W + 1) EPS32 sum_j |w_j g_j|,
  compared per direction slab at the scattered token position.
K4 dw / db.  One partial row is, per lane, a running sum over the at most CONV_CH positions the chunk owns (one product and one
  addition each) followed by the sum of the CONV_BWD_WAVES waves in LDS:
      |row - ref row| <= (CONV_CH + CONV_BWD_WAVES + 2) EPS32 sum |terms| + sum of the terms' own E_g |x|      (db: x = 1).
  Through the C ABI each partial row is compared with the fp64 sum over exactly the positions that workgroup owns (and the rows'
  fp64 total with the autograd gradient); through hip_ops.gather_conv1d_bwd, which ends in a column sum over R partial rows in
  fp32, the factor grows by R EPS32 (any summation order of R terms).
K9.  A lane sums the squares of at most 4 ceil(C / 256) <= ceil(C / 64) + 3 values, then the 6-step wave sum: relative error of the
  sum of squares <= (ceil(C / 64) + 12) EPS32 < GAM_C = 4 (ceil(C / 64) + 8) EPS32, the constant of test_block_ops_gpu.py.  The
  division, the addition of eps and rsqrtf (<= 2 ulp) act on that: |rstd / ref - 1| <= E_R = GAM_C + 4 EPS32 (rsqrt halves the
  argument's error; the bound keeps all of it).
      out = w sum_k y_k rstd_k (K products, K additions, one product):  u |ref| + TINY + (E_R + (K + 2) EPS32) |w| sum_k |y_k| rstd_k.
      dy_k = rstd_k g w - y_k rstd_k^3 <g w, y_k> / C, term by term: the first term carries rstd's error and three roundings, the
      dot product a row reduction (GAM_C sum_c |g w y_k|), its coefficient three more factors of rstd and the division:
        u |ref| + TINY + |rstd g w| (E_R + 4 EPS32) + |y_k| rstd^3 / C * sum_c |g w y_k| * (GAM_C + 3 E_R + 6 EPS32).
      dw partial row: per wave a running sum over RMS_ROWS_PER_BLOCK / 4 rows x K slabs of g y rstd (two products, one addition),
      then 4 waves in LDS: (K RMS_ROWS_PER_BLOCK / 4 + 8) EPS32 + E_R, times sum |g y rstd| over the rows of the group; the test adds
      nothing in fp32.  Through hip_ops.rmsnorm_merge_bwd (column sum over nblk partial rows) the factor grows by nblk EPS32.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
CODE = {F32: 0, BF16: 1, F16: 2}
EPS32 = 2.0 ** -24
UNIT = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}
TINY = {F32: 0.0, BF16: 0.0, F16: 2.0 ** -24}
DM_OK, DM_ERR_ARG, DM_ERR_LAYOUT, DM_ERR_DTYPE = 0, -1, -2, -3
DM_FLAG_SILU = 2
CONV_CH, CONV_BWD_WAVES = 14, 7            # csrc/conv.hip: time steps per chunk, chunks per backward workgroup
CONV_SEG = CONV_CH * CONV_BWD_WAVES        # positions per dw / db partial row
RMS_ROWS_PER_BLOCK = 16                    # csrc/rmsnorm.hip (checked against dm_rmsnorm_merge_rows_per_block())
C_SILU, C_DSILU = 8.0, 11.0
CONV_PART = (CONV_CH + CONV_BWD_WAVES + 2) * EPS32
SENT = 7.0
NAN = float("nan")
IO_W = [(F32, F32), (BF16, F32), (BF16, BF16), (F16, F32), (F16, F16)]
IO_W_IDS = ["f32", "bf16-w32", "bf16-wbf16", "f16-w32", "f16-wf16"]


def _gam_c(C):
    return 4 * (math.ceil(C / 64) + 8) * EPS32


def _lib():
    from diffma_amd import _lib as L

    return L


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _raw(name, a):
    """Status code of one C-ABI call (no exception: the argument-check cases compare it)."""
    return int(getattr(_lib().load(), name)(ctypes.byref(a), _stream()))


def _ok(name, a):
    rc = _raw(name, a)
    if rc != DM_OK:
        raise _lib().DiffmaHipError(f"{name} -> {rc}: {_lib().load().dm_last_error().decode()}")


def _ok_n(name, structs):
    arr = (type(structs[0]) * len(structs))(*structs)
    rc = int(getattr(_lib().load(), name)(ctypes.cast(arr, ctypes.c_void_p), len(structs), _stream()))
    if rc != DM_OK:
        raise _lib().DiffmaHipError(f"{name} -> {rc}: {_lib().load().dm_last_error().decode()}")


def _check(name, got, ref, tol):
    """Per-element |got - ref| <= tol (NaN in got -- an element the kernel never wrote -- fails)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {ref.numel()} elements out of bound; first at flat {i}: "
                             f"got {float(got.flatten()[i])} ref {float(ref.flatten()[i])} tol {float(tol.flatten()[i])}")


def _place(gpu, shape, dt, mode, host=None):
    """A [S, L, D] device view (channel stride 1) inside a buffer filled with the sentinel.  The view holds `host`, or NaN for an output.
    contig; mid: the middle column block of a wider row (both offsets even: the 2-channel form stays); padded: row stride D + 4;
    oddstride: row stride D + 1; oddstart: a dense view that starts one element into its buffer."""
    S, L, D = shape
    if mode == "contig":
        buf = torch.full((S, L, D), SENT, dtype=dt, device=gpu)
        view = buf
    elif mode == "mid":
        buf = torch.full((S, L, D + 12), SENT, dtype=dt, device=gpu)
        view = buf[..., 6:6 + D]
    elif mode == "padded":
        buf = torch.full((S, L, D + 4), SENT, dtype=dt, device=gpu)
        view = buf[..., :D]
    elif mode == "oddstride":
        buf = torch.full((S, L, D + 1), SENT, dtype=dt, device=gpu)
        view = buf[..., :D]
    elif mode == "oddstart":
        buf = torch.full((S * L * D + 1,), SENT, dtype=dt, device=gpu)
        view = buf[1:].view(S, L, D)
    else:
        raise ValueError(mode)
    if host is None:
        view.fill_(NAN)
    else:
        view.copy_(host.to(gpu))
    return buf, view


def _outside_untouched(buf, view):
    chk = buf.clone()
    chk.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(SENT)
    return bool((chk == SENT).all())


# =====================================================================================================================================
# K3 / K4: dm_gather_conv1d_fwd / dm_gather_conv1d_bwd
# =====================================================================================================================================
def _conv_host(B, L, D, W, ndir=1, table=None, iodt=F32, wdt=F32, silu=True, bias=True, wide=False, zero_rows=False, seed=0):
    """Host values, rounded to their storage dtypes.  |pre| stays below 80 by construction (the clamps): the kernel's exp2 has no
    range fix-up and the bounds assume finite intermediates.  wide: |pre| reaches past 30 on both sides."""
    g = torch.Generator().manual_seed(seed)
    table = (ndir > 1) if table is None else table
    assert table or ndir == 1
    S = ndir * B
    if wide:
        x = (torch.randn(B, L, D, generator=g) * 1.3).clamp(-2.4, 2.4)
        w = 8.0 * (torch.randn(D, W, generator=g) * 0.6).clamp(-1.0, 1.0)
    else:
        x = (torch.randn(B, L, D, generator=g) * 1.2).clamp(-4.0, 4.0)
        amp = torch.tensor([0.3, 1.0, 2.5])[torch.arange(D) % 3]
        w = (torch.randn(D, W, generator=g) * 0.5).clamp(-1.5, 1.5) * amp[:, None]
    h = dict(B=B, L=L, D=D, W=W, ndir=ndir, S=S, iodt=iodt, wdt=wdt, silu=silu)
    h["x"] = x.to(iodt)
    h["w"] = w.to(wdt)
    h["b"] = (torch.randn(D, generator=g) * 0.3).to(wdt) if bias else None
    if table:
        rows = ([] if ndir == 1 else [torch.arange(L)]) + [torch.randperm(L, generator=g) for _ in range(ndir - 1 if ndir > 1 else 1)]
        h["idx"] = torch.stack(rows).to(torch.int32)
    else:
        h["idx"] = None
    dout = torch.randn(S, L, D, generator=g)
    if zero_rows:
        dout[:, ::5] = 0.0
    h["dout"] = dout.to(iodt)
    return h


def _conv_reference(h):
    """fp64 reference and per-element bounds (module docstring) of everything K3 / K4 produce."""
    from oracle.mamba_ref import causal_conv1d_ref

    B, L, D, W, ndir, S, silu = (h[k] for k in ("B", "L", "D", "W", "ndir", "S", "silu"))
    u, tiny = UNIT[h["iodt"]], TINY[h["iodt"]]
    idx = h["idx"].long() if h["idx"] is not None else torch.arange(L)[None]
    x64 = h["x"].double().requires_grad_(True)
    w64 = h["w"].double().requires_grad_(True)
    b64 = h["b"].double().requires_grad_(True) if h["b"] is not None else None
    do64 = h["dout"].double()
    xs = torch.cat([x64[:, idx[k]] for k in range(ndir)], 0)                          # [S, L, D], s = dir * B + b
    y = causal_conv1d_ref(xs.permute(0, 2, 1), w64, b64, activation="silu" if silu else None).permute(0, 2, 1)
    leaves = (x64, w64) + ((b64,) if b64 is not None else ())
    dx, dw, db = [], 0.0, 0.0
    for k in range(ndir):                                                             # one backward per direction: dx per slab
        sl = slice(k * B, (k + 1) * B)
        gr = torch.autograd.grad((y[sl] * do64[sl]).sum(), leaves, retain_graph=True)
        dx.append(gr[0])
        dw = dw + gr[1]
        db = db + (gr[2] if b64 is not None else 0.0)
    r = dict(out=y.detach(), dx=torch.cat(dx, 0), dw=dw, db=db if b64 is not None else None)
    with torch.no_grad():
        wa = w64.detach()
        ba = b64.detach() if b64 is not None else torch.zeros(D, dtype=torch.float64)
        pad = torch.cat([torch.zeros(S, W - 1, D, dtype=torch.float64), xs.detach()], 1)  # tap k of position l reads pad[:, l + k]
        pre = ba + sum(wa[:, k] * pad[:, k:k + L] for k in range(W))
        P = ba.abs() + sum((wa[:, k] * pad[:, k:k + L]).abs() for k in range(W))
        E_pre = (W + 2) * EPS32 * P
        if silu:
            sg = torch.sigmoid(pre)
            assert torch.allclose(pre * sg, r["out"], rtol=1e-12, atol=1e-13 * float(P.max() + 1))
            r["tol_out"] = u * r["out"].abs() + tiny + 1.1 * E_pre + C_SILU * (1 + pre.abs()) * EPS32 * r["out"].abs()
            gg = do64 * sg * (1 + pre * (1 - sg))
            E_g = do64.abs() * (0.5 * E_pre + C_DSILU * (1 + pre.abs()) * EPS32)
        else:
            assert torch.allclose(pre, r["out"], rtol=1e-12, atol=1e-13 * float(P.max() + 1))
            r["tol_out"] = u * r["out"].abs() + tiny + E_pre
            gg = do64
            E_g = torch.zeros_like(do64)
        r["pre"] = pre
        # dx in scan order: dxs[m] = sum_j w_j g[m + W-1 - j]; bound terms scattered to token order
        zpad = torch.zeros(S, W - 1, D, dtype=torch.float64)
        gpa, Epa = torch.cat([gg.abs(), zpad], 1), torch.cat([E_g, zpad], 1)
        t_scan = sum(wa[:, W - 1 - k].abs() * (Epa[:, k:k + L] + (W + 1) * EPS32 * gpa[:, k:k + L]) for k in range(W))
        t_tok = torch.empty_like(t_scan)
        for k in range(ndir):
            t_tok[k * B:(k + 1) * B, idx[k]] = t_scan[k * B:(k + 1) * B]
        r["tol_dx"] = u * r["dx"].abs() + tiny + t_tok
        # dw / db partial rows: positions [wg * 98, (wg + 1) * 98) of sequence s
        nchunk = (L + CONV_SEG - 1) // CONV_SEG

        def seg(t):
            tp = torch.cat([t, t.new_zeros(S, nchunk * CONV_SEG - L, D)], 1)
            return tp.view(S, nchunk, CONV_SEG, D).sum(2)

        r["nchunk"] = nchunk
        r["dw_rows"] = torch.stack([seg(gg * pad[:, k:k + L]) for k in range(W)], -1)            # [S, nchunk, D, W]
        r["dw_abs"] = torch.stack([seg((gg * pad[:, k:k + L]).abs()) for k in range(W)], -1)
        r["dw_eg"] = torch.stack([seg(E_g * pad[:, k:k + L].abs()) for k in range(W)], -1)
        r["db_rows"], r["db_abs"], r["db_eg"] = seg(gg), seg(gg.abs()), seg(E_g)
        # the hand-written row sums are the autograd gradients, split by workgroup
        assert torch.allclose(r["dw_rows"].sum((0, 1)), r["dw"], rtol=1e-10, atol=1e-12 * float(r["dw_abs"].sum((0, 1)).max() + 1))
        if r["db"] is not None:
            assert torch.allclose(r["db_rows"].sum((0, 1)), r["db"], rtol=1e-10, atol=1e-12 * float(r["db_abs"].sum((0, 1)).max() + 1))
    return r


def _conv_device(gpu, h, x_mode="contig", do_mode="contig", dx_mode="contig", out_mode=None, part="dense"):
    """Device buffers in the chosen layouts and the two argument structs."""
    L_ = _lib()
    B, L, D, W, ndir, S = (h[k] for k in ("B", "L", "D", "W", "ndir", "S"))
    out_mode = dx_mode if out_mode is None else out_mode
    d = dict(part=part)
    d["xbuf"], d["x"] = _place(gpu, (B, L, D), h["iodt"], x_mode, h["x"])
    d["dobuf"], d["dout"] = _place(gpu, (S, L, D), h["iodt"], do_mode, h["dout"])
    d["outbuf"], d["out"] = _place(gpu, (S, L, D), h["iodt"], out_mode)
    d["dxbuf"], d["dx"] = _place(gpu, (S, L, D), h["iodt"], dx_mode)
    d["w"] = h["w"].to(gpu).contiguous()
    d["b"] = h["b"].to(gpu) if h["b"] is not None else None
    d["idx"] = h["idx"].to(gpu).contiguous() if h["idx"] is not None else None
    d["x_before"] = d["xbuf"].clone()
    nchunk = int(L_.load().dm_conv_nchunk(L))
    assert nchunk == (L + CONV_SEG - 1) // CONV_SEG
    R = S * nchunk
    d["R"], d["nchunk"] = R, nchunk
    if part in ("dense", "dense_nodb"):
        d["dwp"] = torch.full((R, D * W), NAN, device=gpu)
        d["dbp"] = torch.full((R, D), NAN, device=gpu) if part == "dense" else None
        part_ss, dw_ptr, db_ptr = 0, d["dwp"].data_ptr(), (d["dbp"].data_ptr() if part == "dense" else 0)
    else:                                       # dw | db rows in ONE buffer, as the wrapper lays them out; ss_wide: 4 more columns
        extra = 4 if part == "ss_wide" else 0
        d["joint"] = torch.full((R, D * (W + 1) + extra), SENT, device=gpu)
        d["joint"][:, :D * (W + 1)] = NAN
        part_ss, dw_ptr, db_ptr = D * (W + 1) + extra, d["joint"].data_ptr(), d["joint"].data_ptr() + 4 * D * W

    fa = L_.dm_conv_fwd_args()
    fa.batch, fa.dim, fa.seqlen, fa.width, fa.ndir = B, D, L, W, ndir
    fa.io_dtype, fa.w_dtype = CODE[h["iodt"]], CODE[h["wdt"]]
    fa.flags = DM_FLAG_SILU if h["silu"] else 0
    fa.x, fa.weight, fa.bias = d["x"].data_ptr(), d["w"].data_ptr(), (d["b"].data_ptr() if d["b"] is not None else 0)
    fa.row_index = d["idx"].data_ptr() if d["idx"] is not None else 0
    fa.out = d["out"].data_ptr()
    fa.x_sb, fa.x_sl, fa.x_sd = d["x"].stride()
    fa.o_ss, fa.o_sl, fa.o_sd = d["out"].stride()
    ba = L_.dm_conv_bwd_args()
    ba.batch, ba.dim, ba.seqlen, ba.width, ba.ndir = B, D, L, W, ndir
    ba.io_dtype, ba.w_dtype, ba.flags, ba.nchunk = fa.io_dtype, fa.w_dtype, fa.flags, nchunk
    ba.x, ba.weight, ba.bias, ba.dout, ba.row_index = fa.x, fa.weight, fa.bias, d["dout"].data_ptr(), fa.row_index
    ba.dx, ba.dw_partial, ba.db_partial = d["dx"].data_ptr(), dw_ptr, db_ptr
    ba.x_sb, ba.x_sl, ba.x_sd = d["x"].stride()
    ba.do_ss, ba.do_sl, ba.do_sd = d["dout"].stride()
    ba.dx_ss, ba.dx_sl, ba.dx_sd = d["dx"].stride()
    ba.part_ss = part_ss
    d["fa"], d["ba"] = fa, ba
    return d


def _conv_verify(h, d, r, fwd=True, bwd=True):
    B, L, D, W, S = (h[k] for k in ("B", "L", "D", "W", "S"))
    assert torch.equal(d["xbuf"], d["x_before"]), "x is read-only"
    if fwd:
        _check("out", d["out"], r["out"], r["tol_out"])
        assert _outside_untouched(d["outbuf"], d["out"]), "out: written outside the view"
    if not bwd:
        return
    _check("dx (per direction slab)", d["dx"], r["dx"], r["tol_dx"])
    assert _outside_untouched(d["dxbuf"], d["dx"]), "dx: written outside the view"
    nchunk, part = d["nchunk"], d["part"]
    if part in ("dense", "dense_nodb"):
        dwp = d["dwp"].view(S, nchunk, D, W)
        dbp = d["dbp"].view(S, nchunk, D) if part == "dense" else None
    else:
        j = d["joint"]
        dwp = j[:, :D * W].reshape(S, nchunk, D, W)
        dbp = j[:, D * W:D * (W + 1)].reshape(S, nchunk, D)
        assert bool((j[:, D * (W + 1):] == SENT).all()), "partial rows: written past the row"
    _check("dw partial rows", dwp, r["dw_rows"], CONV_PART * r["dw_abs"] + r["dw_eg"])
    _check("dw", dwp.double().sum((0, 1)), r["dw"], (CONV_PART * r["dw_abs"] + r["dw_eg"]).sum((0, 1)))
    if dbp is not None:
        _check("db partial rows", dbp, r["db_rows"], CONV_PART * r["db_abs"] + r["db_eg"])
        if r["db"] is not None:
            _check("db", dbp.double().sum((0, 1)), r["db"], (CONV_PART * r["db_abs"] + r["db_eg"]).sum((0, 1)))


def _conv_run(gpu, B, L, D, W, x_mode="contig", do_mode="contig", dx_mode="contig", out_mode=None, part="dense", **kw):
    """Forward and backward on the same inputs through the C ABI, everything compared with fp64."""
    h = _conv_host(B, L, D, W, **kw)
    d = _conv_device(gpu, h, x_mode, do_mode, dx_mode, out_mode, part)
    _ok("dm_gather_conv1d_fwd", d["fa"])
    _ok("dm_gather_conv1d_bwd", d["ba"])
    torch.cuda.synchronize()
    r = _conv_reference(h)
    _conv_verify(h, d, r)
    return h, r


@pytest.mark.parametrize("W", [2, 3, 4])
@pytest.mark.parametrize("iodt,wdt", IO_W, ids=IO_W_IDS)
def test_conv_dtypes_vs_fp64(gpu, iodt, wdt, W):
    """fp32; bf16 and fp16 each with fp32 weights and with weights in the I/O dtype (TW = bf16_t / f16_t); every width.  66 channels:
    the 2-channel form (VEC 2) with a partial wave; 3 directions, 33 steps (three chunks, the last one partial)."""
    _conv_run(gpu, 2, 33, 66, W, ndir=3, iodt=iodt, wdt=wdt, seed=100 + W)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("dirs", ["1", "1table", "2", "3", "4"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("silu", [True, False], ids=["silu", "linear"])
def test_conv_flag_arms_vs_fp64(gpu, silu, bias, dirs, batch):
    """SILU on / off, bias / NULL, ndir 1 with row_index = NULL, ndir 1 with a (non-identity) table, ndir 2..4, batch 1 and 3;
    fp32 and bf16 (VEC 2) each.  db partial rows are written and compared also when bias is NULL."""
    ndir = int(dirs[0])
    for iodt in (F32, BF16):
        _conv_run(gpu, batch, 29, 64, 4, ndir=ndir, table=(dirs != "1"), iodt=iodt, silu=silu, bias=bias, seed=110 + ndir + batch)


@pytest.mark.parametrize("L", [1, 2, 3, 13, 14, 15, 98, 99, 112, 196, 197, 225])
def test_conv_lengths_vs_fp64(gpu, L):
    """Shorter than the window (1, 2, 3), chunk boundaries (13, 14, 15), workgroup boundaries (98, 99: a second workgroup whose
    waves 1..6 hold empty chunks; 112; 196, 197: three workgroups; 225).  fp32, bf16, fp16; 2 directions, batch 2."""
    for iodt in (F32, BF16, F16):
        _conv_run(gpu, 2, L, 64, 4, ndir=2, iodt=iodt, seed=120 + L)
    _conv_run(gpu, 1, L, 6, 3, ndir=1, iodt=BF16, wdt=BF16, seed=121 + L)


@pytest.mark.parametrize("D", [2, 64, 66, 128, 200, 1056, 1, 63, 201])
def test_conv_widths_vs_fp64(gpu, D):
    """Channel counts: even ones take the 2-channel form in 16 bits (2: one lane; 66, 200, 1056: a partial last wave; 1056 is the
    Mamba-2 xBC width at hidden size 512), odd ones (1, 63, 201) the one-channel-per-lane fallback.  fp32, bf16, fp16."""
    for iodt in (F32, BF16, F16):
        _conv_run(gpu, 2, 30, D, 4, ndir=2, iodt=iodt, seed=130 + D)


@pytest.mark.parametrize("how", ["oddstride", "oddstart"])
@pytest.mark.parametrize("which", ["x", "dout", "dx_out"])
@pytest.mark.parametrize("iodt", [BF16, F16], ids=["bf16", "f16"])
def test_conv_vec1_fallback_vs_fp64(gpu, iodt, which, how):
    """16-bit I/O, even dim, and exactly ONE of x, dout, dx / out with an odd row stride or starting at an odd element: the launch
    must take VEC = 1 (a 32-bit access there would straddle elements).  With dout alone the forward still runs VEC = 2."""
    modes = dict(x_mode="contig", do_mode="contig", dx_mode="contig")
    modes[{"x": "x_mode", "dout": "do_mode", "dx_out": "dx_mode"}[which]] = how
    _conv_run(gpu, 2, 30, 66, 4, ndir=3, iodt=iodt, seed=140, **modes)
    _conv_run(gpu, 1, 17, 66, 3, ndir=1, iodt=iodt, wdt=iodt, bias=False, seed=141, **modes)


@pytest.mark.parametrize("part", ["dense", "dense_nodb", "ss", "ss_wide"])
@pytest.mark.parametrize("iodt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_conv_layouts_vs_fp64(gpu, iodt, part):
    """x as the middle column block of a wider row (the zxbcdt[..., Din:Din + Cx] view), dout, out and dx with a row stride above
    dim (sentinel padding that must survive); partial rows dense (part_ss = 0), dense with db_partial = NULL, in the wrapper's joint
    dw | db buffer (part_ss = dim (W + 1)) and in a joint buffer with a wider row stride.  99 steps: two workgroups per sequence."""
    _conv_run(gpu, 2, 99, 64, 4, ndir=3, iodt=iodt, x_mode="mid", do_mode="padded", dx_mode="padded", part=part, seed=150)
    _conv_run(gpu, 1, 20, 6, 2, ndir=2, iodt=iodt, x_mode="mid", do_mode="mid", dx_mode="mid", out_mode="padded", part=part, seed=151)


@pytest.mark.parametrize("iodt,wdt", IO_W, ids=IO_W_IDS)
def test_conv_values_vs_fp64(gpu, iodt, wdt):
    """pre spread past +-30 (both tails of silu' and the exp2 range), every fifth dout row zero; 197 steps (three workgroups)."""
    h, r = _conv_run(gpu, 1, 197, 128, 4, ndir=2, iodt=iodt, wdt=wdt, wide=True, zero_rows=True, seed=160)
    assert float(r["pre"].min()) < -30 and float(r["pre"].max()) > 30 and float(r["pre"].abs().max()) < 80
    _conv_run(gpu, 1, 60, 64, 2, ndir=1, iodt=iodt, wdt=wdt, wide=True, zero_rows=True, silu=False, seed=161)


def test_conv_wrappers_mamba2_shape_vs_fp64(gpu):
    """hip_ops.gather_conv1d_fwd / _bwd at the Mamba-2 shape of hidden size 512: bf16, xBC = 1056 channels read as the middle
    column block of zxbcdt, L = 196, 3 directions, fp32 weights; `out=` a strided view.  dw / db come back column-summed in fp32
    over R = ndir * B * nchunk partial rows: R EPS32 on top of the partial-row factor."""
    from diffma_amd import hip_ops

    B, L, D, W, ndir, Din = 2, 196, 1056, 4, 3, 1024
    h = _conv_host(B, L, D, W, ndir=ndir, iodt=BF16, seed=170)
    g = torch.Generator().manual_seed(171)
    zx = torch.randn(B, L, Din + D + 16, generator=g).to(BF16)
    zx[..., Din:Din + D] = h["x"]
    zxd = zx.to(gpu)
    xv = zxd[..., Din:Din + D]
    obuf = torch.full((ndir * B, L, D + 8), SENT, dtype=BF16, device=gpu)
    ov = obuf[..., :D]
    ov.fill_(NAN)
    wd, bd, idxd = h["w"].to(gpu), h["b"].to(gpu), h["idx"].to(gpu)
    out = hip_ops.gather_conv1d_fwd(xv, wd, bd, row_index=idxd, ndir=ndir, silu=True, out=ov)
    dx, dw, db = hip_ops.gather_conv1d_bwd(xv, wd, bd, h["dout"].to(gpu), row_index=idxd, ndir=ndir, silu=True)
    torch.cuda.synchronize()
    assert out.data_ptr() == ov.data_ptr() and bool((obuf[..., D:] == SENT).all())
    assert torch.equal(zxd.cpu(), zx)
    r = _conv_reference(h)
    _check("out", out, r["out"], r["tol_out"])
    _check("dx (per direction slab)", dx, r["dx"], r["tol_dx"])
    fac = CONV_PART + ndir * B * r["nchunk"] * EPS32
    assert dw.dtype == db.dtype == F32
    _check("dw", dw, r["dw"], (fac * r["dw_abs"] + r["dw_eg"]).sum((0, 1)))
    _check("db", db, r["db"], (fac * r["db_abs"] + r["db_eg"]).sum((0, 1)))


@pytest.mark.parametrize("dt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("act", ["silu", None], ids=["silu", "linear"])
def test_causal_conv1d_fn_forward_and_autograd_vs_fp64(gpu, act, bias, dt):
    """The drop-in causal_conv1d_fn in the reference's (B, D, L) layout: forward and torch.autograd.grad (x, weight, bias) against
    fp64.  bf16: x, weight and bias all bf16, so dweight / dbias are rounded once more into bf16 (u of their value on top)."""
    from diffma_amd.selective_scan_interface import causal_conv1d_fn

    B, L, D, W = 2, 50, 96, 4
    h = _conv_host(B, L, D, W, iodt=dt, wdt=dt, silu=act is not None, bias=bias, seed=180)
    x = h["x"].permute(0, 2, 1).contiguous().to(gpu).requires_grad_(True)              # (B, D, L), L contiguous
    w = h["w"].to(gpu).requires_grad_(True)
    b = h["b"].to(gpu).requires_grad_(True) if bias else None
    dout = h["dout"].permute(0, 2, 1).contiguous().to(gpu)
    out = causal_conv1d_fn(x, w, b, activation=act)
    assert out.shape == (B, D, L) and out.dtype == dt
    grads = torch.autograd.grad(out, (x, w) + ((b,) if bias else ()), dout)
    torch.cuda.synchronize()
    r = _conv_reference(h)
    _check("out", out.permute(0, 2, 1), r["out"], r["tol_out"])
    assert grads[0].shape == (B, D, L) and grads[0].dtype == dt
    _check("dx", grads[0].permute(0, 2, 1), r["dx"], r["tol_dx"])
    fac = CONV_PART + B * r["nchunk"] * EPS32
    assert grads[1].dtype == dt and grads[1].shape == (D, W)
    _check("dweight", grads[1], r["dw"], (fac * r["dw_abs"] + r["dw_eg"]).sum((0, 1)) + UNIT[dt] * r["dw"].abs() + TINY[dt])
    if bias:
        assert grads[2].dtype == dt
        _check("dbias", grads[2], r["db"], (fac * r["db_abs"] + r["db_eg"]).sum((0, 1)) + UNIT[dt] * r["db"].abs() + TINY[dt])


@pytest.mark.parametrize("odd_first", [False, True], ids=["aligned-odd", "odd-aligned"])
@pytest.mark.parametrize("iodt", [BF16, F16], ids=["bf16", "f16"])
def test_conv_pair_entry_with_different_alignment(gpu, iodt, odd_first):
    """dm_gather_conv1d_fwd_n / _bwd_n with two structs that are congruent in every size and stride but whose x (forward and
    backward) and dx (backward) differ in 4-byte alignment, so that one takes VEC = 2 and the other VEC = 1: the same_align4 rule must
    keep them out of one grid.  Both results are right against fp64 and equal, bit for bit, to two single calls."""
    hs = [_conv_host(2, 30, 64, 4, ndir=3, iodt=iodt, seed=190 + i) for i in range(2)]
    lay = [dict(x_mode="contig", dx_mode="contig"), dict(x_mode="oddstart", dx_mode="oddstart")]
    if odd_first:
        lay.reverse()
    pair = [_conv_device(gpu, hs[i], out_mode="contig", **lay[i]) for i in range(2)]
    single = [_conv_device(gpu, hs[i], out_mode="contig", **lay[i]) for i in range(2)]
    assert pair[0]["x"].stride() == pair[1]["x"].stride() and (pair[0]["x"].data_ptr() ^ pair[1]["x"].data_ptr()) & 3
    _ok_n("dm_gather_conv1d_fwd_n", [p["fa"] for p in pair])
    _ok_n("dm_gather_conv1d_bwd_n", [p["ba"] for p in pair])
    for s in single:
        _ok("dm_gather_conv1d_fwd", s["fa"])
        _ok("dm_gather_conv1d_bwd", s["ba"])
    torch.cuda.synchronize()
    for i in range(2):
        r = _conv_reference(hs[i])
        _conv_verify(hs[i], pair[i], r)
        for name in ("out", "dx", "dwp", "dbp"):
            assert torch.equal(pair[i][name], single[i][name]), (i, name)


def test_conv_argument_checks(gpu):
    """Rejections by return code, nothing launched: null pointers, sizes <= 0, ndir > 1 without a table, a channel stride != 1, widths
    1 and 5, a w_dtype that is neither fp32 nor the I/O dtype, an unknown io_dtype, a wrong nchunk, ndir * batch over the grid limit.
    The unmodified structs are accepted."""
    h = _conv_host(1, 4, 8, 4, iodt=BF16, seed=200)
    h["x"].zero_()
    h["dout"].zero_()
    d = _conv_device(gpu, h)
    bufs = [d[k] for k in ("xbuf", "dobuf", "outbuf", "dxbuf", "dwp", "dbp")]
    idx = torch.zeros(4 * 4, dtype=torch.int32, device=gpu)
    assert _raw("dm_gather_conv1d_fwd", d["fa"]) == DM_OK and _raw("dm_gather_conv1d_bwd", d["ba"]) == DM_OK
    torch.cuda.synchronize()
    before = [t.clone() for t in bufs]                    # what the accepted calls left; no rejected call may change it
    assert not any(bool(torch.isnan(t.float()).any()) for t in before)

    def variant(base, **kw):
        a = type(base)()
        ctypes.memmove(ctypes.byref(a), ctypes.byref(base), ctypes.sizeof(base))
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for name, base in (("dm_gather_conv1d_fwd", d["fa"]), ("dm_gather_conv1d_bwd", d["ba"])):
        bwd = name.endswith("bwd")
        assert int(getattr(_lib().load(), name)(None, _stream())) == DM_ERR_ARG
        for f in ("x", "weight") + (("dout", "dx", "dw_partial") if bwd else ("out",)):
            assert _raw(name, variant(base, **{f: 0})) == DM_ERR_ARG, (name, f)
        for f in ("batch", "dim", "seqlen", "ndir"):
            for v in (0, -1):
                assert _raw(name, variant(base, **{f: v})) == DM_ERR_ARG, (name, f, v)
        assert _raw(name, variant(base, ndir=2)) == DM_ERR_ARG                          # no table
        assert _raw(name, variant(base, ndir=1, row_index=idx.data_ptr())) == DM_OK     # (a table with ndir = 1 is accepted)
        for f in ("x_sd",) + (("do_sd", "dx_sd") if bwd else ("o_sd",)):
            assert _raw(name, variant(base, **{f: 2})) == DM_ERR_LAYOUT, (name, f)
        for wd in (1, 5):
            assert _raw(name, variant(base, width=wd)) == DM_ERR_ARG, (name, wd)
        assert _raw(name, variant(base, w_dtype=CODE[F16])) == DM_ERR_DTYPE             # io bf16, weights fp16
        assert _raw(name, variant(base, io_dtype=CODE[F32], w_dtype=CODE[BF16])) == DM_ERR_DTYPE
        assert _raw(name, variant(base, io_dtype=3, w_dtype=3)) == DM_ERR_DTYPE
        assert _raw(name, variant(base, batch=32768)) == DM_ERR_ARG                     # 2 * ndir * batch > 65535 grid planes
        if bwd:
            for nc in (0, 2):
                assert _raw(name, variant(base, nchunk=nc)) == DM_ERR_ARG, nc
    torch.cuda.synchronize()
    for t, b in zip(bufs, before):
        assert torch.equal(t, b)


# =====================================================================================================================================
# K9: dm_rmsnorm_merge_fwd / dm_rmsnorm_merge_bwd
# =====================================================================================================================================
def _rms_host(K, R, C, dt, rows="randn", seed=0):
    g = torch.Generator().manual_seed(seed)
    y = torch.randn(K, R, C, generator=g) * 1.5
    if rows == "mixed":                         # rows of magnitude 1.5, exactly zero, 1e3 and 1e-3, different per slab
        sc = torch.tensor([1.5, 0.0, 1e3, 1e-3])
        y = torch.randn(K, R, C, generator=g) * sc[(torch.arange(R)[None, :] + torch.arange(K)[:, None]) % 4][..., None]
    elif rows == "small":
        y = torch.randn(K, R, C, generator=g) * 1e-3
    w = 1 + 0.5 * torch.randn(C, generator=g)
    dout = torch.randn(R, C, generator=g)
    return dict(K=K, R=R, C=C, dt=dt, y=y.to(dt), w=w.float(), dout=dout.to(dt))


def _rms_reference(h, eps):
    K, R, C, dt = h["K"], h["R"], h["C"], h["dt"]
    u, tiny = UNIT[dt], TINY[dt]
    eps = float(torch.tensor(eps, dtype=F32))                                         # the value the fp32 struct field holds
    y = h["y"].double().requires_grad_(True)
    w = h["w"].double().requires_grad_(True)
    g = h["dout"].double()
    rstd = torch.rsqrt(y.pow(2).mean(-1, keepdim=True) + eps)
    out = (y * rstd).sum(0) * w
    dy, dw = torch.autograd.grad((out * g).sum(), (y, w))
    with torch.no_grad():
        gc = _gam_c(C)
        E_R = gc + 4 * EPS32
        rs, ya, wa = rstd.detach(), y.detach(), w.detach()
        r = dict(out=out.detach(), rstd=rs[..., 0], dy=dy, dw=dw)
        r["tol_rstd"] = rs[..., 0] * E_R
        r["tol_out"] = u * r["out"].abs() + tiny + (E_R + (K + 2) * EPS32) * wa.abs() * (ya.abs() * rs).sum(0)
        gw = g * wa
        Dsum = (gw * ya).abs().sum(-1, keepdim=True)
        r["tol_dy"] = (u * dy.abs() + tiny + (rs * gw).abs() * (E_R + 4 * EPS32)
                       + ya.abs() * rs ** 3 / C * Dsum * (gc + 3 * E_R + 6 * EPS32))
        nblk = (R + RMS_ROWS_PER_BLOCK - 1) // RMS_ROWS_PER_BLOCK
        terms = g * ya * rs                                                            # [K, R, C]

        def seg(t):
            tp = torch.cat([t, t.new_zeros(K, nblk * RMS_ROWS_PER_BLOCK - R, C)], 1)
            return tp.view(K, nblk, RMS_ROWS_PER_BLOCK, C).sum((0, 2))

        r["nblk"] = nblk
        r["dw_rows"], r["dw_abs"] = seg(terms), seg(terms.abs())
        r["dw_fac"] = (K * RMS_ROWS_PER_BLOCK / 4 + 8) * EPS32 + E_R
        assert torch.allclose(r["dw_rows"].sum(0), dw, rtol=1e-10, atol=1e-12 * float(r["dw_abs"].sum(0).max() + 1))
    return r


def _rms_run(gpu, K, R, C, dt, eps=1e-5, rows="randn", strided=False, seed=0):
    L_ = _lib()
    assert int(L_.load().dm_rmsnorm_merge_rows_per_block()) == RMS_ROWS_PER_BLOCK
    h = _rms_host(K, R, C, dt, rows, seed)
    py, po, pg, pd = (8, 4, 12, 4) if strided else (0, 0, 0, 0)           # row padding of y, out, dout, dy; y / dy also get spare rows
    xr = 1 if strided else 0
    ybuf = torch.full((K, R + xr, C + py), SENT, dtype=dt, device=gpu)
    yv = ybuf[:, :R, :C]
    yv.copy_(h["y"].to(gpu))
    y_before = ybuf.clone()
    obuf = torch.full((R, C + po), SENT, dtype=dt, device=gpu)
    ov = obuf[:, :C]
    ov.fill_(NAN)
    gbuf = torch.full((R, C + pg), SENT, dtype=dt, device=gpu)
    gv = gbuf[:, :C]
    gv.copy_(h["dout"].to(gpu))
    dbuf = torch.full((K, R + 2 * xr, C + pd), SENT, dtype=dt, device=gpu)
    dv = dbuf[:, :R, :C]
    dv.fill_(NAN)
    wd = h["w"].to(gpu)
    rstd = torch.full((K, R), NAN, device=gpu)
    nblk = (R + RMS_ROWS_PER_BLOCK - 1) // RMS_ROWS_PER_BLOCK
    part = torch.full((nblk, C), NAN, device=gpu)
    a = L_.dm_rmsnorm_merge_args()
    a.nslab, a.C, a.rows, a.io_dtype, a.eps = K, C, R, CODE[dt], eps
    a.y, a.weight, a.out, a.rstd = yv.data_ptr(), wd.data_ptr(), ov.data_ptr(), rstd.data_ptr()
    a.y_ss, a.y_sr, a.out_sr = yv.stride(0), yv.stride(1), ov.stride(0)
    _ok("dm_rmsnorm_merge_fwd", a)
    a.dout, a.dy, a.dw_part = gv.data_ptr(), dv.data_ptr(), part.data_ptr()
    a.dout_sr, a.dy_ss, a.dy_sr = gv.stride(0), dv.stride(0), dv.stride(1)
    _ok("dm_rmsnorm_merge_bwd", a)
    torch.cuda.synchronize()
    r = _rms_reference(h, eps)
    assert torch.equal(ybuf, y_before), "y is read-only"
    _check("rstd", rstd, r["rstd"], r["tol_rstd"])
    _check("out", ov, r["out"], r["tol_out"])
    _check("dy", dv, r["dy"], r["tol_dy"])
    _check("dw partial rows", part, r["dw_rows"], r["dw_fac"] * r["dw_abs"])
    _check("dw", part.double().sum(0), r["dw"], r["dw_fac"] * r["dw_abs"].sum(0))
    if strided:
        assert bool((obuf[:, C:] == SENT).all()), "out: written past the row"
        assert bool((dbuf[:, :, C:] == SENT).all()) and bool((dbuf[:, R:] == SENT).all()), "dy: written outside the view"
    return r


@pytest.mark.parametrize("C", [4, 200, 1024, 1028, 2048, 2304, 3076, 4096])
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_rms_widths_vs_fp64(gpu, dt, C):
    """Every NIT instantiation at both ends: 4 (C = 4, 200, 1024), 8 (1028, 2048), 12 (2304), 16 (3076, 4096); fp32, bf16, fp16;
    K = 3, 5 rows (one partial 16-row group, a partial 4-row forward workgroup)."""
    _rms_run(gpu, 3, 5, C, dt, seed=300 + C)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_rms_slab_counts_vs_fp64(gpu, dt, K):
    """K = 1 (route A), 2 (ViM), 3 (spiral), 4 (VMamba) at a NIT 4 and a NIT 8 width."""
    _rms_run(gpu, K, 7, 200, dt, seed=310 + K)
    _rms_run(gpu, K, 18, 1028, dt, seed=311 + K)


@pytest.mark.parametrize("Bsz", [1, 3])
@pytest.mark.parametrize("rows", [1, 3, 4, 5, 15, 16, 17, 70])
def test_rms_row_counts_vs_fp64(gpu, rows, Bsz):
    """Row counts around the forward workgroup (4 rows) and the backward group (16 rows), times Bsz 1 and 3; fp32 and bf16."""
    for dt in (F32, BF16):
        _rms_run(gpu, 3, rows * Bsz, 260, dt, seed=320 + rows)


@pytest.mark.parametrize("C", [200, 2048, 4096])
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_rms_strided_vs_fp64(gpu, dt, C):
    """Slabs, out, dout and dy with row strides above C (each its own) and slab strides above rows * row stride; the sentinel
    padding comes back unchanged."""
    _rms_run(gpu, 3, 19, C, dt, strided=True, seed=330 + C)
    _rms_run(gpu, 2, 16, C, dt, strided=True, seed=331 + C)


@pytest.mark.parametrize("case", ["mixed", "mixed_eps_large", "small_eps_large", "small"])
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_rms_values_vs_fp64(gpu, dt, case):
    """Zero rows (rstd = eps^-1/2, out = 0, dy = rstd g w), rows of magnitude 1e3 and 1e-3 in one launch; rows of 1e-3 next to
    eps = 0.1 (eps outside the root or added to the rms is far off) and next to eps = 1e-5."""
    rows = "mixed" if case.startswith("mixed") else "small"
    eps = 0.1 if case.endswith("eps_large") else 1e-5
    _rms_run(gpu, 3, 21, 200, dt, eps=eps, rows=rows, seed=340)
    _rms_run(gpu, 2, 9, 1028, dt, eps=eps, rows=rows, strided=True, seed=341)


@pytest.mark.parametrize("K,Bsz,L,C", [(3, 2, 49, 1024), (1, 1, 5, 200), (4, 3, 17, 2304), (2, 3, 70, 64)])
@pytest.mark.parametrize("dt", [F32, BF16, F16], ids=["f32", "bf16", "f16"])
def test_rms_wrappers_vs_fp64(gpu, dt, K, Bsz, L, C):
    """hip_ops.rmsnorm_merge_fwd / _bwd on [K, B, L, C] slabs; the weight gradient comes back column-summed in fp32 over nblk
    partial rows: nblk EPS32 on top of the partial-row factor."""
    from diffma_amd import hip_ops

    eps = 1e-5
    h = _rms_host(K, Bsz * L, C, dt, seed=350 + C)
    yd = h["y"].view(K, Bsz, L, C).to(gpu)
    out, rstd = hip_ops.rmsnorm_merge_fwd(yd, h["w"].to(gpu), eps)
    dy, dw = hip_ops.rmsnorm_merge_bwd(yd, h["w"].to(gpu), eps, rstd, h["dout"].view(Bsz, L, C).to(gpu))
    torch.cuda.synchronize()
    r = _rms_reference(h, eps)
    assert out.shape == (Bsz, L, C) and dy.shape == (K, Bsz, L, C) and out.dtype == dy.dtype == dt and dw.dtype == F32
    _check("rstd", rstd, r["rstd"], r["tol_rstd"])
    _check("out", out.view(-1, C), r["out"], r["tol_out"])
    _check("dy", dy.view(K, -1, C), r["dy"], r["tol_dy"])
    _check("dw", dw, r["dw"], (r["dw_fac"] + r["nblk"] * EPS32) * r["dw_abs"].sum(0))


def test_rms_argument_checks(gpu):
    """Rejections by return code, nothing launched: C % 4, C > 4096, sizes <= 0, a stride that is not a multiple of 4, a pointer off
    16 bytes, null pointers, an unknown dtype.  The unmodified struct is accepted."""
    L_ = _lib()
    K, R, C = 2, 3, 8
    y = torch.zeros(K, R, C + 8, device=gpu)
    out, dout, dy = torch.zeros(R, C + 8, device=gpu), torch.zeros(R, C + 8, device=gpu), torch.zeros(K, R, C + 8, device=gpu)
    w, rstd, part = torch.zeros(4200, device=gpu), torch.zeros(K * R, device=gpu), torch.zeros(4200, device=gpu)

    def args(**kw):
        a = L_.dm_rmsnorm_merge_args()
        a.nslab, a.C, a.rows, a.io_dtype, a.eps = K, C, R, 0, 1e-5
        a.y, a.weight, a.out, a.rstd = y.data_ptr(), w.data_ptr(), out.data_ptr(), rstd.data_ptr()
        a.dout, a.dy, a.dw_part = dout.data_ptr(), dy.data_ptr(), part.data_ptr()
        a.y_ss, a.y_sr, a.out_sr, a.dout_sr, a.dy_ss, a.dy_sr = R * (C + 8), C + 8, C + 8, C + 8, R * (C + 8), C + 8
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert _raw("dm_rmsnorm_merge_fwd", args()) == DM_OK and _raw("dm_rmsnorm_merge_bwd", args()) == DM_OK
    torch.cuda.synchronize()
    bufs = (y, out, dout, dy, rstd, part)
    before = [t.clone() for t in bufs]                    # what the accepted calls left; no rejected call may change it
    for name in ("dm_rmsnorm_merge_fwd", "dm_rmsnorm_merge_bwd"):
        bwd = name.endswith("bwd")
        assert int(getattr(L_.load(), name)(None, _stream())) == DM_ERR_ARG
        for cbad in (6, 4100, 0, -4):
            assert _raw(name, args(C=cbad)) == DM_ERR_ARG, (name, cbad)
        for f in ("nslab", "rows"):
            for v in (0, -1):
                assert _raw(name, args(**{f: v})) == DM_ERR_ARG, (name, f, v)
        for f in ("y", "weight", "rstd") + (("dout", "dy", "dw_part") if bwd else ("out",)):
            assert _raw(name, args(**{f: 0})) == DM_ERR_ARG, (name, f)
        for f in ("y_ss", "y_sr", "out_sr", "dout_sr", "dy_ss", "dy_sr"):
            assert _raw(name, args(**{f: C + 10})) == DM_ERR_LAYOUT, (name, f)
        for f, t in (("y", y), ("weight", w)) + ((("dout", dout), ("dy", dy), ("dw_part", part)) if bwd else (("out", out),)):
            assert _raw(name, args(**{f: t.data_ptr() + 4})) == DM_ERR_LAYOUT, (name, f)
        assert _raw(name, args(io_dtype=3)) == DM_ERR_DTYPE
    torch.cuda.synchronize()
    for t, b in zip(bufs, before):
        assert torch.equal(t, b)
