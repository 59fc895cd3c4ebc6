"""csrc/conv_xproj.hip (K3x forward; K4x backward: per-sequence, whole-sample merged and persistent slab forms) and csrc/dtproj.hip (K8,
K8b) per element against fp64: bitwise on integer inputs, within derived bounds on real ones.

Builders, fp64 references, bound functions -- with their derivations -- and the emulations are in tests/test_conv_xproj_dtproj_cpu.py;
the kernels' outputs go through the same `*_eval` functions as the emulations there.  The launches go through the C ABI with hand-built
structs (strides, NULL pointers, part_ss, nblk and DM_FLAG_PARTIAL_COMPACT are the test's choice); one test per entry point goes
through the hip_ops wrappers as well.  Layouts: x and dx are the x half of a [.., L, 2 D] buffer whose z half holds a sentinel; du rows
have a padded stride; x_dbl / dx_dbl rows have stride 72 with the columns past the projection width holding a sentinel (outputs) or NaN
(inputs: they must not be read); every output view is pre-filled with NaN, so an element the kernel never wrote fails its comparison.

Largest error-to-bound ratio on the MI355X when this file was written (test_zz_error_to_bound_ratios prints them under -s):
    xproj_fwd        bf16 0.995  fp16 0.996
    xproj_bwd_seq    bf16 0.988  fp16 0.951        its dw / db (.dwdb)  bf16 0.009  fp16 0.013
    xproj_bwd_whole  bf16 0.966  fp16 0.924        its dw / db          bf16 0.017  fp16 0.018
    xproj_bwd_slab   bf16 0.980  fp16 0.944        its dw / db          bf16 0.006  fp16 0.008
    dtproj_fwd       bf16 0.994  fp16 0.989
    dtproj_bwd       bf16 0.861  fp16 0.474        its dW (.dW)         bf16 0.015  fp16 0.034
(16-bit outputs: the output's own half-ulp rounding, the same elements as in the emulation; the fp32 reductions are booked apart.)
"""
import ctypes

import pytest
import torch

from tests.test_block_ops_gpu import _ok, _raw
from tests.test_conv_xproj_dtproj_cpu import (DB_SHAPES, DT_SHAPES, IO, IO_IDS, NPROJ_B, RATIOS, SENT, XB_SEQ_SHAPES, XB_SLAB_SHAPES,
                                              XB_THRESHOLD_L, XB_WHOLE_SHAPES, XP_IDS, XP_SHAPES, _ids, db_case, db_eval, db_nblks,
                                              dt_case, dt_eval, xb_case, xb_chain, xb_eval, xb_merged_case, xp_case, xp_eval)
from tests.test_mixer_passes_cpu import BF16, CODE, DM_ERR_ARG, DM_ERR_DTYPE, DM_ERR_LAYOUT, DM_OK, F16, F32, NAN
from tests.test_mixer_passes_gpu import _frame, _intact

pytestmark = pytest.mark.gpu


def _half(gpu, dt, n, L, D, fill=None):
    """The x half of a [n, L, 2 D] buffer whose z half holds the sentinel; NaN in the view unless `fill` is given."""
    buf = torch.full((n, L, 2 * D), SENT, dtype=dt, device=gpu)
    view = buf[..., :D]
    if fill is None:
        view.fill_(NAN)
    else:
        view.copy_(fill)
    return buf, view


def _z_intact(buf, D, what):
    assert bool((buf[..., D:] == SENT).all()), f"{what}: the z half next to the view was written"


def _conv_common(gpu, c, a, keep):
    """Fields the forward and the backward struct share: sizes, x, conv parameters, row tables."""
    xbuf, x = _half(gpu, c.dt, c.B, c.L, c.D, c.x)
    w = c.w.to(gpu).contiguous()
    bias = None if c.bias is None else c.bias.to(gpu).contiguous()
    idx = None if c.idx is None else c.idx.to(gpu).contiguous()
    keep += [xbuf, w, bias, idx]
    a.batch, a.dim, a.seqlen, a.width, a.ndir = c.B, c.D, c.L, c.W, c.ndir
    a.io_dtype, a.w_dtype = CODE[c.dt], CODE[c.w.dtype]
    a.x, a.weight = x.data_ptr(), w.data_ptr()
    a.bias = None if bias is None else bias.data_ptr()
    a.row_index = None if idx is None else idx.data_ptr()
    a.x_sb, a.x_sl, a.x_sd = x.stride()
    return x, w, bias, idx


# =====================================================================================================================================
# K3x
# =====================================================================================================================================
def _xp_build(gpu, c):
    from diffma_amd._lib import DM_FLAG_SILU, dm_conv_xproj_fwd_args

    a, keep = dm_conv_xproj_fwd_args(), []
    _conv_common(gpu, c, a, keep)
    S = c.ndir * c.B
    obuf, out = _half(gpu, c.dt, S, c.L, c.D)
    xdbl = torch.full((S * c.L, c.xd_sr), SENT, dtype=c.dt, device=gpu)
    xdbl[:, :c.P] = NAN
    wx = c.wx.to(gpu).contiguous()
    keep.append(wx)
    a.flags = DM_FLAG_SILU if c.silu else 0
    a.nproj = c.P
    a.wx, a.out, a.xdbl = wx.data_ptr(), out.data_ptr(), xdbl.data_ptr()
    a.o_ss, a.o_sl, a.o_sd = out.stride()
    a.xd_sr = c.xd_sr
    return a, keep, obuf, out, xdbl


def _xp_run(gpu, c):
    a, keep, obuf, out, xdbl = _xp_build(gpu, c)
    _ok("dm_gather_conv1d_xproj_fwd", a)
    torch.cuda.synchronize()
    _z_intact(obuf, c.D, "x~")
    _z_intact(keep[0], c.D, "x")
    return xp_eval(c, out, xdbl, book=RATIOS)


@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
@pytest.mark.parametrize("shape", XP_SHAPES, ids=XP_IDS)
def test_xproj_fwd_exact_on_integers(gpu, dt, shape):
    """K3x, silu off, integer operands: x~ and x_dbl bit for bit; conv widths 2 / 3 / 4, with and without row tables, ndir 1 and 3, conv
    weights in fp32 and in the I/O dtype, bias present and NULL, nproj 1 .. 64 in rows of stride 72."""
    _xp_run(gpu, xp_case(dt, *shape, "int", seed=1000 + XP_SHAPES.index(shape)))


@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
@pytest.mark.parametrize("shape", XP_SHAPES, ids=XP_IDS)
def test_xproj_fwd_within_derived_bounds(gpu, dt, shape):
    """K3x with SiLU on real values: x~ against fp64, x_dbl against the fp64 product of the kernel's own x~."""
    _xp_run(gpu, xp_case(dt, *shape, "real", seed=1000 + XP_SHAPES.index(shape)))


@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
@pytest.mark.parametrize("mode", ["int", "real"])
def test_xproj_fwd_through_the_wrapper(gpu, dt, mode):
    """hip_ops.gather_conv1d_xproj_fwd (dense x_dbl rows) on three of the shapes, through the same evaluation."""
    from diffma_amd import hip_ops

    for i in (5, 6, 12):
        c = xp_case(dt, *XP_SHAPES[i], mode, seed=1000 + i)
        xbuf, x = _half(gpu, dt, c.B, c.L, c.D, c.x)
        xc, xdbl = hip_ops.gather_conv1d_xproj_fwd(x, c.w.to(gpu), None if c.bias is None else c.bias.to(gpu), c.wx.to(gpu),
                                                   row_index=None if c.idx is None else c.idx.to(gpu), ndir=c.ndir, silu=c.silu)
        torch.cuda.synchronize()
        frame = torch.full((xdbl.shape[0], c.xd_sr), SENT, dtype=dt)
        frame[:, :c.P] = xdbl.cpu()
        xp_eval(c, xc, frame, book=RATIOS)


# =====================================================================================================================================
# K4x
# =====================================================================================================================================
def _xb_build(gpu, c, variant=0, compact=False):
    """variant 0: dw | db rows in one buffer (part_ss); 1: two dense buffers (part_ss = 0); 2: db_partial == NULL."""
    from diffma_amd._lib import DM_FLAG_DX_MERGED, DM_FLAG_PARTIAL_COMPACT, DM_FLAG_SILU, dm_conv_xproj_bwd_args

    a, keep = dm_conv_xproj_bwd_args(), []
    _conv_common(gpu, c, a, keep)
    S, D, W, L = c.ndir * c.B, c.D, c.W, c.L
    dubuf, du = _frame(gpu, c.dt, (S, L, D), (L * (D + 8) + 16, D + 8, 1), 8, c.du.view(S, L, D))
    dxd = torch.full((S * L, 72), NAN, dtype=c.dt, device=gpu)
    dxd[:, :NPROJ_B] = c.dxdbl.to(gpu)
    wxt = c.wxt.to(gpu).contiguous()
    dxbuf, dx = _half(gpu, c.dt, c.B if c.merged else S, L, D)
    keep += [dubuf, du, dxd, wxt]
    a.flags = (DM_FLAG_SILU if c.silu else 0) | (DM_FLAG_DX_MERGED if c.merged else 0) | (DM_FLAG_PARTIAL_COMPACT if compact else 0)
    a.nproj = NPROJ_B
    a.du, a.dxdbl, a.wxt, a.dx = du.data_ptr(), dxd.data_ptr(), wxt.data_ptr(), dx.data_ptr()
    a.du_ss, a.du_sl, a.du_sd = du.stride()
    a.dx_ss, a.dx_sl, a.dx_sd = dx.stride()
    a.xd_sr = 72
    rows = c.B if c.merged else S
    if variant == 0:
        part = torch.full((rows, D * (W + 1)), NAN, dtype=F32, device=gpu)
        dwp, dbp = part[:, :D * W], part[:, D * W:]
        a.part_ss = D * (W + 1)
    else:
        dwp = torch.full((rows, D * W), NAN, dtype=F32, device=gpu)
        dbp = torch.full((rows, D), NAN, dtype=F32, device=gpu) if variant == 1 else None
        a.part_ss = 0
    a.dw_partial = dwp.data_ptr()
    a.db_partial = None if dbp is None else dbp.data_ptr()
    return a, keep, dxbuf, dx, dwp, dbp


def _xb_run(gpu, c, variant=0, compact=False, evaluate=True):
    """Launch, check the frames, evaluate.  Slab form: dm_gather_conv1d_xproj_bwd_slab() names the R partial rows that carry sums; the
    rows R .. batch - 1 are zero (and harmless in the sum), or untouched under DM_FLAG_PARTIAL_COMPACT."""
    from diffma_amd import _lib

    a, keep, dxbuf, dx, dwp, dbp = _xb_build(gpu, c, variant, compact)
    R = int(_lib.load().dm_gather_conv1d_xproj_bwd_slab(ctypes.byref(a), None))
    assert (R > 0) == (c.form == "slab"), f"the launch took the {'slab' if R else 'tiled'} form, the case is built for {c.form}"
    _ok("dm_gather_conv1d_xproj_bwd", a)
    torch.cuda.synchronize()
    _z_intact(dxbuf, c.D, "dx")
    _intact(keep[4], keep[5], "du")
    if R:
        assert 0 < R <= c.B
        for p in (dwp, dbp):
            if p is not None:
                assert bool(p[R:].isnan().all() if compact else (p[R:] == 0).all()), "partial rows past the ones that carry sums"
        dwp, dbp = dwp[:R], None if dbp is None else dbp[:R]
    if evaluate:
        xb_eval(c, dx, dwp, dbp, chain=xb_chain(c, R), book=RATIOS)
    return R, dx, dwp, dbp


@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
@pytest.mark.parametrize("mode", ["int", "real"])
@pytest.mark.parametrize("shape", XB_SEQ_SHAPES, ids=_ids(XB_SEQ_SHAPES))
def test_xproj_bwd_per_sequence(gpu, monkeypatch, dt, mode, shape):
    """K4x, one workgroup per gathered sequence.  "int": silu off, dx per direction, dw and db bit for bit (integer-valued fp32 sums of
    the partial rows); "real": SiLU, every element within its bound.  The three partial-row layouts take turns."""
    monkeypatch.delenv("DM_K4X_SLAB", raising=False)
    i = XB_SEQ_SHAPES.index(shape)
    _xb_run(gpu, xb_case(dt, "seq", *shape, mode, seed=2000 + i), variant=i % 3)


@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
@pytest.mark.parametrize("mode", ["int", "seq", "real"])
@pytest.mark.parametrize("shape", XB_WHOLE_SHAPES, ids=_ids(XB_WHOLE_SHAPES))
def test_xproj_bwd_whole_sample(gpu, monkeypatch, dt, mode, shape):
    """K4x with DM_FLAG_DX_MERGED, whole-sample form (DM_K4X_SLAB=0).  "int" / "seq": SiLU saturated by bias 64 (silu' == 1.0f), the
    running sum over the directions, dw and db bit for bit -- "seq" with sums that leave the exact range of the I/O dtype, so that the
    rounding per direction shows; "real": within the bounds."""
    monkeypatch.setenv("DM_K4X_SLAB", "0")
    i = XB_WHOLE_SHAPES.index(shape)
    _xb_run(gpu, xb_merged_case(dt, "whole", shape, mode, (3500 if mode == "seq" else 3000) + i), variant=i % 3)


@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
@pytest.mark.parametrize("mode", ["int", "seq", "real"])
@pytest.mark.parametrize("shape", XB_SLAB_SHAPES, ids=_ids(XB_SLAB_SHAPES))
def test_xproj_bwd_slab(gpu, monkeypatch, dt, mode, shape):
    """The slab form (DM_K4X_SLAB=1): 8 segments with recomputed halo rows, 14- and 16-row tiles, waves with empty segments, token 255
    in the byte table, ndir 1 / 3 / 4; both DM_FLAG_PARTIAL_COMPACT settings take turns with the partial-row layouts."""
    monkeypatch.setenv("DM_K4X_SLAB", "1")
    i = XB_SLAB_SHAPES.index(shape)
    _xb_run(gpu, xb_merged_case(dt, "slab", shape, mode, (3500 if mode == "seq" else 3000) + i), variant=i % 3, compact=(i // 3) % 2 == 1)


@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
@pytest.mark.parametrize("L", XB_THRESHOLD_L)
def test_xproj_bwd_merged_at_the_default_threshold(gpu, monkeypatch, dt, L):
    """DM_K4X_SLAB unset: 31 rows take the whole-sample form, 32 and 33 the slab form (_xb_run asserts which one ran); exact either way."""
    monkeypatch.delenv("DM_K4X_SLAB", raising=False)
    form = "slab" if L >= 32 else "whole"
    for mode in ("int", "real"):
        _xb_run(gpu, xb_merged_case(dt, form, (2, L, 256, 3, False), mode, 3700 + L))


@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
def test_xproj_bwd_slab_workgroups_walk_two_samples(gpu, monkeypatch, dt):
    """dim 1024, L 32 and a batch 8 above the number of partial rows dm_gather_conv1d_xproj_bwd_slab() reports for a large batch: one
    workgroup stream in each XCD walks two samples, sums their dw | db in registers and, without DM_FLAG_PARTIAL_COMPACT, zero-fills
    the second sample's row.  Both flag settings give the same dx and the same rows, bit for bit."""
    from diffma_amd import _lib
    from diffma_amd._lib import DM_FLAG_DX_MERGED, DM_FLAG_SILU, dm_conv_xproj_bwd_args

    monkeypatch.setenv("DM_K4X_SLAB", "1")
    probe = dm_conv_xproj_bwd_args()
    probe.batch, probe.dim, probe.seqlen, probe.width, probe.ndir = 1 << 20, 1024, 32, 4, 3
    probe.flags = DM_FLAG_SILU | DM_FLAG_DX_MERGED
    probe.row_index = 64                                                            # (not read: the answer depends on sizes and alignment)
    probe.dx_ss, probe.dx_sl = 32 * 2048, 2048
    full = int(_lib.load().dm_gather_conv1d_xproj_bwd_slab(ctypes.byref(probe), None))
    assert full >= 8 and full % 8 == 0
    c = xb_merged_case(dt, "slab", (full + 8, 32, 1024, 3, False), "int", 3800)
    R0, dx0, dw0, db0 = _xb_run(gpu, c, variant=0, compact=False)
    R1, dx1, dw1, db1 = _xb_run(gpu, c, variant=0, compact=True, evaluate=False)
    assert R0 == R1 == full
    assert torch.equal(dx0, dx1) and torch.equal(dw0, dw1) and torch.equal(db0, db1)


@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
@pytest.mark.parametrize("slab", ["0", "1"])
def test_xproj_bwd_through_the_wrapper(gpu, monkeypatch, dt, slab):
    """hip_ops.gather_conv1d_xproj_bwd, per direction and merged: the wrapper's own partial-row bookkeeping and column sum."""
    from diffma_amd import hip_ops

    monkeypatch.setenv("DM_K4X_SLAB", slab)
    for form, shape, mode in (("seq", XB_SEQ_SHAPES[5], "int"), ("seq", XB_SEQ_SHAPES[9], "real"),
                              ("merged", (2, 33, 128, 4, False), "int"), ("merged", (2, 33, 128, 4, False), "real")):
        if form == "seq":
            c = xb_case(dt, "seq", *shape, mode, seed=2100)
        else:
            c = xb_merged_case(dt, "slab" if slab == "1" else "whole", shape, mode, 3900)
        xbuf, x = _half(gpu, dt, c.B, c.L, c.D, c.x)
        dxbuf, dxm = _half(gpu, dt, c.B, c.L, c.D)
        dx, dw, db = hip_ops.gather_conv1d_xproj_bwd(x, c.w.to(gpu), None if c.bias is None else c.bias.to(gpu), c.du.to(gpu),
                                                     c.dxdbl.to(gpu), c.wxt.to(gpu), row_index=None if c.idx is None else c.idx.to(gpu),
                                                     ndir=c.ndir, silu=c.silu, merged_out=dxm if c.merged else None)
        torch.cuda.synchronize()
        _z_intact(dxbuf, c.D, "dx")
        # the wrapper's column sum is one more fp32 pass over the partial rows: its rows are charged to the chain
        xb_eval(c, dx, dw, db, chain=xb_chain(c) + c.ndir * c.B + 20, book=RATIOS)


# =====================================================================================================================================
# K8 / K8b
# =====================================================================================================================================
def _dt_run(gpu, c):
    from diffma_amd._lib import dm_dtproj_args

    xd = c.xdbl.to(gpu)
    w = c.w.to(gpu).contiguous()
    bias = None if c.bias is None else c.bias.to(gpu)
    obuf, out = _frame(gpu, c.dt, (c.M, c.Dm), (c.Dm, 1), 8)
    a = dm_dtproj_args()
    a.rows, a.dim, a.rank, a.io_dtype = c.M, c.Dm, c.R, CODE[c.dt]
    a.xdbl, a.w, a.delta = xd.data_ptr(), w.data_ptr(), out.data_ptr()
    a.bias = None if bias is None else bias.data_ptr()
    a.xd_sr = c.xd_sr
    _ok("dm_dtproj_softplus_fwd", a)
    torch.cuda.synchronize()
    _intact(obuf, out, "delta")
    return dt_eval(c, out, book=RATIOS)


@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
@pytest.mark.parametrize("mode", ["int", "real", "band"])
@pytest.mark.parametrize("shape", DT_SHAPES, ids=_ids(DT_SHAPES))
def test_dtproj_softplus(gpu, dt, mode, shape):
    """K8.  "int": pre >= 21, the x > 20 branch returns the rounded pre bit for bit (column permutation, rank mask, row tails, the
    128-byte store path without the softplus); "real" / "band": the three branches within their bounds.  The x_dbl columns past the
    rank hold NaN and the rows have a stride above the rank."""
    i = DT_SHAPES.index(shape)
    _dt_run(gpu, dt_case(dt, *shape, (i % 5) != 0, mode, seed=4000 + i))


def _db_run(gpu, c, nblk):
    from diffma_amd._lib import dm_dtproj_bwd_args

    dd, xd, w = c.dd.to(gpu).contiguous(), c.xdbl.to(gpu), c.w.to(gpu).contiguous()
    dxd = torch.full((c.M, c.dxd_sr), SENT, dtype=c.dt, device=gpu)
    dxd[:, :c.R] = NAN
    pbuf, part = _frame(gpu, F32, (nblk, c.Dm * c.R), (c.Dm * c.R, 1), 8)
    a = dm_dtproj_bwd_args()
    a.rows, a.dim, a.rank, a.io_dtype, a.nblk = c.M, c.Dm, c.R, CODE[c.dt], nblk
    a.ddelta, a.xdbl, a.w, a.dxdbl, a.part = dd.data_ptr(), xd.data_ptr(), w.data_ptr(), dxd.data_ptr(), part.data_ptr()
    a.xd_sr, a.dxd_sr = c.xd_sr, c.dxd_sr
    _ok("dm_dtproj_bwd", a)
    torch.cuda.synchronize()
    _intact(pbuf, part, "part")
    return db_eval(c, dxd, part, book=RATIOS)


@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
@pytest.mark.parametrize("mode", ["int", "real"])
@pytest.mark.parametrize("shape", DB_SHAPES, ids=_ids(DB_SHAPES))
def test_dtproj_bwd(gpu, dt, mode, shape):
    """K8b, every instantiation (512 / 768 / 1024 x rank 16 / 32), rows 1 .. 95, nblk 1, 2 and ceil(rows / 32): dxdbl[:, :R] and dW (the
    partial images added in fp64) bit for bit on integers and within the GEMM-form bounds on real values; the columns past the rank of
    the stride-64 dxdbl rows keep their sentinel."""
    c = db_case(dt, *shape, mode, seed=5000 + DB_SHAPES.index(shape))
    for nblk in db_nblks(c.M):
        _db_run(gpu, c, nblk)


@pytest.mark.parametrize("dt", IO, ids=IO_IDS)
def test_dtproj_through_the_wrappers(gpu, dt):
    from diffma_amd import hip_ops

    c = dt_case(dt, 33, 272, 24, True, "real", seed=4100)
    dt_eval(c, hip_ops.dtproj_softplus_fwd(c.xdbl.to(gpu), c.w.to(gpu), c.bias.to(gpu)), book=RATIOS)
    for mode in ("int", "real"):
        c = db_case(dt, 95, 768, 32, mode, seed=5100)
        dxd = torch.full((c.M, c.dxd_sr), SENT, dtype=dt, device=gpu)
        dW = hip_ops.dtproj_bwd(c.dd.to(gpu), c.xdbl.to(gpu), c.w.to(gpu), dxd)
        torch.cuda.synchronize()
        db_eval(c, dxd, dW, book=RATIOS)


# =====================================================================================================================================
# status codes: each refusal is the documented DM_ERR_* and leaves the outputs untouched
# =====================================================================================================================================
def _refused(name, a, want, outs):
    assert _raw(name, a) == want, (name, want)
    torch.cuda.synchronize()
    for t in outs:
        if t is not None:
            assert bool(t.isnan().all()), f"{name}: a refused call wrote an output"


def test_xproj_fwd_status_codes(gpu):
    def build(**kw):
        c = xp_case(BF16, 1, 5, kw.pop("D", 128), kw.pop("P", 64), 4, kw.pop("ndir", 1), True, False, True, "real", seed=1)
        a, keep, obuf, out, xdbl = _xp_build(gpu, c)
        xdbl.fill_(NAN)
        return a, keep, [out, xdbl]

    a, keep, outs = build()
    assert _raw("dm_gather_conv1d_xproj_fwd", a) == DM_OK
    for field, value, want in [("dim", 192, DM_ERR_ARG), ("nproj", 65, DM_ERR_ARG), ("nproj", 0, DM_ERR_ARG), ("width", 5, DM_ERR_ARG),
                               ("x_sl", 257, DM_ERR_LAYOUT), ("o_sl", 257, DM_ERR_LAYOUT), ("o_sd", 2, DM_ERR_LAYOUT),
                               ("w_dtype", CODE[F16], DM_ERR_DTYPE), ("io_dtype", CODE[F32], DM_ERR_ARG)]:
        a, keep, outs = build()
        setattr(a, field, value)
        _refused("dm_gather_conv1d_xproj_fwd", a, want, outs)
    a, keep, outs = build(ndir=3)
    a.row_index = None
    _refused("dm_gather_conv1d_xproj_fwd", a, DM_ERR_ARG, outs)


def test_xproj_bwd_status_codes(gpu, monkeypatch):
    from diffma_amd._lib import DM_FLAG_DX_MERGED, DM_FLAG_PARTIAL_COMPACT

    monkeypatch.setenv("DM_K4X_SLAB", "0")

    def build(W=4, ndir=1, merged=False):
        if merged:
            c = xb_merged_case(BF16, "whole", (1, 5, 128, ndir, False), "real", 1)
        else:
            c = xb_case(BF16, "seq", 1, 5, 128, W, ndir, True, False, True, "real", seed=1)
        a, keep, dxbuf, dx, dwp, dbp = _xb_build(gpu, c)
        return a, keep, [dx, dwp, dbp]

    a, keep, outs = build()
    assert _raw("dm_gather_conv1d_xproj_bwd", a) == DM_OK
    for field, value, want in [("dim", 192, DM_ERR_ARG), ("nproj", 48, DM_ERR_ARG), ("width", 5, DM_ERR_ARG), ("x_sl", 257, DM_ERR_LAYOUT),
                               ("du_sl", 137, DM_ERR_LAYOUT), ("dx_sl", 257, DM_ERR_LAYOUT), ("xd_sr", 68, DM_ERR_LAYOUT),
                               ("w_dtype", CODE[F16], DM_ERR_DTYPE), ("io_dtype", CODE[F32], DM_ERR_ARG)]:
        a, keep, outs = build()
        setattr(a, field, value)
        _refused("dm_gather_conv1d_xproj_bwd", a, want, outs)
    a, keep, outs = build(ndir=3)
    a.row_index = None
    _refused("dm_gather_conv1d_xproj_bwd", a, DM_ERR_ARG, outs)
    a, keep, outs = build(W=3)
    a.flags |= DM_FLAG_DX_MERGED
    _refused("dm_gather_conv1d_xproj_bwd", a, DM_ERR_ARG, outs)
    a, keep, outs = build(ndir=3, merged=True)                                     # the whole-sample form writes `batch` rows
    a.flags |= DM_FLAG_PARTIAL_COMPACT
    _refused("dm_gather_conv1d_xproj_bwd", a, DM_ERR_ARG, outs)


def test_dtproj_status_codes(gpu):
    from diffma_amd._lib import dm_dtproj_args, dm_dtproj_bwd_args

    M = 40
    x = torch.zeros(M, 48, dtype=BF16, device=gpu)
    w = torch.zeros(1024, 32, dtype=BF16, device=gpu)
    out = torch.full((M, 1024), NAN, dtype=BF16, device=gpu)

    def fwd(**kw):
        a = dm_dtproj_args()
        a.rows, a.dim, a.rank, a.io_dtype = M, 64, 32, CODE[BF16]
        a.xdbl, a.w, a.delta, a.xd_sr = x.data_ptr(), w.data_ptr(), out.data_ptr(), 48
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw, want in [(dict(dim=24), DM_ERR_LAYOUT), (dict(rank=12), DM_ERR_LAYOUT), (dict(rank=40), DM_ERR_LAYOUT),
                     (dict(xd_sr=44), DM_ERR_LAYOUT), (dict(xd_sr=24), DM_ERR_LAYOUT), (dict(io_dtype=CODE[F32]), DM_ERR_LAYOUT),
                     (dict(rows=0), DM_ERR_ARG), (dict(xdbl=x.data_ptr() + 2), DM_ERR_LAYOUT)]:
        _refused("dm_dtproj_softplus_fwd", fwd(**kw), want, [out])
    assert _raw("dm_dtproj_softplus_fwd", fwd()) == DM_OK

    dd = torch.zeros(M, 1024, dtype=BF16, device=gpu)
    dxd = torch.full((M, 64), NAN, dtype=BF16, device=gpu)
    part = torch.full((2, 1024 * 32), NAN, dtype=F32, device=gpu)

    def bwd(**kw):
        a = dm_dtproj_bwd_args()
        a.rows, a.dim, a.rank, a.io_dtype, a.nblk = M, 1024, 32, CODE[BF16], 2
        a.ddelta, a.xdbl, a.w, a.dxdbl, a.part = dd.data_ptr(), x.data_ptr(), w.data_ptr(), dxd.data_ptr(), part.data_ptr()
        a.xd_sr, a.dxd_sr = 48, 64
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    for kw in [dict(dim=256), dict(rank=8), dict(rank=24), dict(nblk=0), dict(nblk=3), dict(xd_sr=44), dict(dxd_sr=66), dict(rows=0),
               dict(io_dtype=CODE[F32])]:
        _refused("dm_dtproj_bwd", bwd(**kw), DM_ERR_ARG, [dxd, part])
    assert _raw("dm_dtproj_bwd", bwd()) == DM_OK


def test_zz_error_to_bound_ratios(gpu):
    """Prints the largest error-to-bound ratio per operator and dtype that the tests of this file have seen so far (run it with -s)."""
    for k in sorted(RATIOS):
        print(f"gpu ratio {k[0]:20s} {k[1]}: {RATIOS[k]:.3f}")
    assert all(v <= 1.0 for v in RATIOS.values())
