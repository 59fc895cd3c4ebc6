"""csrc/merge.hip and csrc/gate_head.hip operator by operator against fp64: dm_token_merge (plain, gated, fp32 to 16-bit), dm_gate_bwd,
dm_sum_partials, dm_colsum_f32, dm_gate_head_fwd / dm_gate_head_bwd and the dm_*_n entries of the first four.

The calls go through the C ABI with hand-built structs, so the strides, the view offsets (and with them the 16-byte or element-wise
instantiation), nblk and every dtype pair are chosen by the test rather than by the wrappers.  Builders, fp64 references and bound
functions -- with their derivations -- are in tests/test_mixer_passes_cpu.py; the kernels' outputs go through the same `*_eval`
functions as the emulations there.  Every output tensor is a view into a larger buffer: the view is pre-filled with NaN (an element
the kernel never wrote fails its bound) and the frame around it with a sentinel that is compared afterwards.

The layouts: a [.., rows, D] tensor starts 8 elements into its buffer and its strides are multiples of 8 with room between the rows, so
everything is 16-byte aligned in all three dtypes; an alignment class bumps ONE offset or stride by one element, which sends the launch
to the element-wise instantiation (launch_merge / launch_gate_bwd: merge.hip:92-96, 176-178).

Largest error-to-bound ratio on the MI355X when this file was written (test_zz_error_to_bound_ratios prints them under -s); what is
left below 1 is the room a rewrite of these kernels has:
    token_merge   fp32 0.373  bf16 0.994  fp16 0.993        gate_bwd       fp32 0.394  bf16 0.989  fp16 0.988
    sum_partials  fp32 1.000  bf16 0.995  fp16 0.993        colsum         fp32 0.129
    gate_head_fwd fp32 0.103  bf16 0.991  fp16 0.987        gate_head_bwd  fp32 0.446  bf16 0.995  fp16 0.979
(16-bit: the output's own half-ulp rounding; sum_partials fp32 at nw = 2 is one rounding against a bound of one rounding.)
"""
import ctypes
from types import SimpleNamespace as NS

import pytest
import torch

from tests.test_block_ops_gpu import _ok, _raw
from tests.test_mixer_passes_cpu import (BF16, CODE, COLSUM_C, COLSUM_R, DM_ERR_ARG, DM_ERR_DTYPE, DM_ERR_LAYOUT, DM_OK, DTYPES, F16,
                                         F32, GH_NBLK, NAME, NAN, RATIOS, VECMAX, bits_equal, colsum_case, colsum_eval, gate_bwd_case,
                                         gate_bwd_cases, gate_bwd_eval, gh_bwd_eval, gh_case, gh_cases, gh_fwd_eval, merge_case,
                                         merge_cases, merge_eval, sum_partials_case, sum_partials_eval)

pytestmark = pytest.mark.gpu

SENT = 7.0
IDS = list(NAME.values())


def _rup(n):
    return -(-n // 8) * 8


def _frame(gpu, dt, shape, strides, off, fill=None):
    """A view of `shape` / `strides` starting `off` elements into a sentinel-filled buffer; NaN in the view unless `fill` is given."""
    span = off + sum((n - 1) * s for n, s in zip(shape, strides)) + 1
    buf = torch.full((span + 16,), SENT, dtype=dt, device=gpu)
    assert buf.data_ptr() % 16 == 0
    view = buf.as_strided(tuple(shape), tuple(strides), off)
    if fill is None:
        view.fill_(NAN)
    else:
        view.copy_(fill)
    return buf, view


def _intact(buf, view, what):
    c = buf.clone()
    c.as_strided(view.shape, view.stride(), view.storage_offset()).fill_(SENT)
    assert bool((c == SENT).all()), f"{what}: the kernel wrote outside its view"


def _untouched(view):
    return bool(view.isnan().all())


def _bld(gpu, dt, B, L, D, bump, name, fill=None, sl0=None):
    """[B, L, D] tensor `name` in the aligned layout, with the bumps of `bump` that name it: name (offset), name_sl, name_sb."""
    sl0 = sl0 or _rup(D) + 8
    sb0 = _rup(L * (sl0 + 1)) + 8
    sl, sb, off = sl0 + (name + "_sl" in bump), sb0 + (name + "_sb" in bump), 8 + (name in bump)
    return _frame(gpu, dt, (B, L, D), (sb, sl, 1), off, fill)


def _raw_n(name, structs, n=None):
    from diffma_amd import _lib

    arr = (type(structs[0]) * len(structs))(*structs)
    return int(getattr(_lib.load(), name + "_n")(ctypes.cast(arr, ctypes.c_void_p), len(structs) if n is None else n,
                                                 ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


# =====================================================================================================================================
# dm_token_merge
# =====================================================================================================================================
def _merge_build(gpu, c, bump=()):
    from diffma_amd._lib import dm_merge_args

    sl0 = _rup(c.D) + 8
    sb0 = _rup(c.L * (sl0 + 1)) + 8
    sk0 = _rup(c.B * (sb0 + 1)) + 8
    sl, sb, sk = sl0 + ("in_sl" in bump), sb0 + ("in_sb" in bump), sk0 + ("in_sk" in bump)
    inbuf, inv = _frame(gpu, c.dt, (c.K, c.B, c.L, c.D), (sk, sb, sl, 1), 8 + ("in" in bump), c.slabs)
    obuf, out = _bld(gpu, c.out_dt, c.B, c.L, c.D, bump, "out")
    m = NS(c=c, keep=[inbuf, inv], obuf=obuf, out=out, pbuf=None, pre=None)
    a = dm_merge_args()
    a.nin, a.batch, a.seqlen, a.dim = c.K, c.B, c.L, c.D
    a.io_dtype, a.out_dtype = CODE[c.dt], CODE[c.out_dt]
    setattr(a, "in", inv.data_ptr())
    a.in_sk, a.in_sb, a.in_sl = sk, sb, sl
    a.out, a.o_sb, a.o_sl = out.data_ptr(), out.stride(0), out.stride(1)
    if c.idx is not None:
        idx = c.idx.to(gpu).contiguous()
        m.keep.append(idx)
        a.row_index = idx.data_ptr()
    if c.gated:
        gbuf, gv = _bld(gpu, c.dt, c.B, c.L, c.D, bump, "gate", c.z)
        m.keep += [gbuf, gv]
        a.gate, a.g_sb, a.g_sl = gv.data_ptr(), gv.stride(0), gv.stride(1)
    if c.want_pre:
        m.pbuf, m.pre = _bld(gpu, c.dt, c.B, c.L, c.D, bump, "pre")
        a.pre, a.p_sb, a.p_sl = m.pre.data_ptr(), m.pre.stride(0), m.pre.stride(1)
    m.a = a
    return m


def _merge_finish(m):
    torch.cuda.synchronize()
    _intact(m.obuf, m.out, "token_merge out")
    if m.pre is not None:
        _intact(m.pbuf, m.pre, "token_merge pre")
    out, pre = m.out.cpu(), (m.pre.cpu() if m.pre is not None else None)
    merge_eval(m.c, out, pre)
    return out, pre


def _merge_run(gpu, c, bump=()):
    m = _merge_build(gpu, c, bump)
    _ok("dm_token_merge", m.a)
    return _merge_finish(m)


MERGE_BUMPS = ["in", "out", "in_sl", "in_sb", "in_sk", "out_sl", "out_sb"]
MERGE_GATED_BUMPS = MERGE_BUMPS + ["gate", "gate_sl", "gate_sb", "pre", "pre_sl", "pre_sb"]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_token_merge_alignment_classes(gpu, dt):
    """B 2, L 5, K 3.  Every class that leaves the 16-byte arm, one at a time, against the all-aligned run of the same values: `pre` and
    the ungated outputs bit-identical between the two (both are the exactly rounded fp32 sequence), the gated outputs within bound.
    dim 1, 7 and 263 are element-wise by themselves; 263 is two workgroups, seven live threads in the second."""
    for D in (1, 7, 263):
        _merge_run(gpu, merge_case(dt, 2, 5, D, 3, seed=D))
        _merge_run(gpu, merge_case(dt, 2, 5, D, 3, gated=True, want_pre=True, table="perm", seed=100 + D))
        _merge_run(gpu, merge_case(dt, 2, 5, D, 3, gated=True, table="perm", seed=200 + D))
    plain = merge_case(dt, 2, 5, 40, 3, table="perm", seed=1)
    gated = merge_case(dt, 2, 5, 40, 3, table="perm", gated=True, want_pre=True, seed=2)
    out0, _ = _merge_run(gpu, plain)
    _, pre0 = _merge_run(gpu, gated)
    for b in MERGE_BUMPS:
        out, _ = _merge_run(gpu, plain, (b,))
        assert bits_equal(out, out0), b
    for b in MERGE_GATED_BUMPS:
        _, pre = _merge_run(gpu, gated, (b,))
        assert bits_equal(pre, pre0), b


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_token_merge_two_blocks_along_dim(gpu, dt):
    """The 16-byte arm with a second workgroup along dim: 257 vectors (dim 1028 fp32, 2056 16-bit), L 3; and the element-wise arm of
    the same width (`in` one element off)."""
    D = 257 * VECMAX[dt]
    for kw in (dict(), dict(gated=True, want_pre=True), dict(gated=True)):
        c = merge_case(dt, 2, 3, D, 2, table="perm", seed=3, **kw)
        _merge_run(gpu, c)
        _merge_run(gpu, c, ("in",))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_token_merge_value_and_table_classes(gpu, dt):
    """nin 1 .. 4; row_index NULL, identity, a permutation per slab, a table with repeated rows (the contract is a gather); the gated
    form with a table, with and without pre; fp32 to bf16 / fp16; z at its edges; cancelling slabs; fp16 subnormal slabs."""
    for c in merge_cases(dt):
        _merge_run(gpu, c)
        if c.D % 8 == 0:
            _merge_run(gpu, c, ("out_sl",))


def test_token_merge_status_codes(gpu):
    c = merge_case(F32, 2, 3, 8, 2, gated=True, want_pre=True, seed=4)

    def args(**kw):
        m = _merge_build(gpu, c)
        for k, v in kw.items():
            setattr(m.a, k, v)
        return m

    cases = [(dict(gate=0), DM_ERR_ARG), (dict(io_dtype=1, out_dtype=0), DM_ERR_DTYPE), (dict(io_dtype=2, out_dtype=1), DM_ERR_DTYPE),
             (dict(io_dtype=0, out_dtype=1), DM_ERR_DTYPE), (dict(out=0), DM_ERR_ARG), (dict(nin=0), DM_ERR_ARG),
             (dict(batch=0), DM_ERR_ARG), (dict(seqlen=-1), DM_ERR_ARG), (dict(dim=0), DM_ERR_ARG), (dict(batch=32768), DM_ERR_ARG),
             (dict(seqlen=65536), DM_ERR_ARG), ({"in": 0}, DM_ERR_ARG)]
    for kw, want in cases:
        m = args(**kw)
        assert _raw("dm_token_merge", m.a) == want, kw
        torch.cuda.synchronize()
        assert _untouched(m.out) and _untouched(m.pre), kw
    m = args(gate=0, pre=0)                                   # ungated: a dtype pair outside the five is DM_ERR_DTYPE
    m.a.io_dtype, m.a.out_dtype = 1, 0
    assert _raw("dm_token_merge", m.a) == DM_ERR_DTYPE
    from diffma_amd import _lib

    assert int(_lib.load().dm_token_merge(None, None)) == DM_ERR_ARG
    _merge_run(gpu, merge_case(F32, 32767, 1, 8, 2, seed=5))    # the largest accepted batch: grid.z = 32767


# =====================================================================================================================================
# dm_gate_bwd
# =====================================================================================================================================
def _gbw_build(gpu, c, bump=(), dz_half=False):
    from diffma_amd._lib import dm_gate_bwd_args

    m = NS(c=c, keep=[])
    a = dm_gate_bwd_args()
    a.batch, a.seqlen, a.dim, a.io_dtype = c.B, c.L, c.D, CODE[c.dt]
    for name, fill in (("dy", c.dy), ("z", c.z), ("pre", c.pre)):
        buf, v = _bld(gpu, c.dt, c.B, c.L, c.D, bump, name, fill)
        m.keep += [buf, v]
        setattr(a, name, v.data_ptr())
        pfx = "p" if name == "pre" else name
        setattr(a, pfx + "_sb", v.stride(0))
        setattr(a, pfx + "_sl", v.stride(1))
    m.gbuf, m.g = _bld(gpu, c.dt, c.B, c.L, c.D, bump, "g")
    if dz_half:                                             # dz = the z half of a d(xz) buffer of row width 2 D; the x half is frame
        m.dzbuf, m.dz = _frame(gpu, c.dt, (c.B, c.L, c.D), (c.L * 2 * c.D, 2 * c.D, 1), c.D)
    else:
        m.dzbuf, m.dz = _bld(gpu, c.dt, c.B, c.L, c.D, bump, "dz")
    a.g, a.g_sb, a.g_sl = m.g.data_ptr(), m.g.stride(0), m.g.stride(1)
    a.dz, a.dz_sb, a.dz_sl = m.dz.data_ptr(), m.dz.stride(0), m.dz.stride(1)
    m.a = a
    return m


def _gbw_finish(m):
    torch.cuda.synchronize()
    _intact(m.gbuf, m.g, "gate_bwd g")
    _intact(m.dzbuf, m.dz, "gate_bwd dz")
    g, dz = m.g.cpu(), m.dz.cpu()
    gate_bwd_eval(m.c, g, dz)
    return g, dz


def _gbw_run(gpu, c, bump=(), dz_half=False):
    m = _gbw_build(gpu, c, bump, dz_half)
    _ok("dm_gate_bwd", m.a)
    return _gbw_finish(m)


GBW_BUMPS = [n + s for n in ("dy", "z", "pre", "g", "dz") for s in ("", "_sl", "_sb")]


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_gate_bwd_alignment_classes_and_values(gpu, dt):
    """dim 1, 7, 263 and every single misaligned pointer or stride of the five tensors (the element-wise arm), each within bound of
    fp64; z over its value classes with pre and dy at magnitudes 1e-3 .. 1e3.  g = (dy z) sg is a chain of products and comes out
    bit-identical to the all-aligned run.  dz does not (fp32 and fp16 differ in the last place on the MI355X): 1 + z (1 - sg) is open
    to contraction into an FMA and the compiler decides per instantiation, so dz is held to its bound only."""
    for c in gate_bwd_cases(dt)[:4]:
        _gbw_run(gpu, c)
    c = gate_bwd_case(dt, 2, 5, 40, seed=6)
    g0, _ = _gbw_run(gpu, c)
    for b in GBW_BUMPS:
        g, _ = _gbw_run(gpu, c, (b,))
        assert bits_equal(g, g0), b


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_gate_bwd_two_blocks_and_xz_half(gpu, dt):
    """257 vectors per row in the 16-byte arm and the same width element-wise; dz into the z half of a d(xz) frame (16-byte arm at
    D = 64, element-wise at D = 7 and D = 263), the x half untouched."""
    c = gate_bwd_cases(dt)[4]
    assert c.D == 257 * 8
    _gbw_run(gpu, c)
    _gbw_run(gpu, c, ("z",))
    for D in (64, 7, 263):
        _gbw_run(gpu, gate_bwd_case(dt, 2, 3, D, seed=7 + D), dz_half=True)


def test_gate_bwd_status_codes(gpu):
    from diffma_amd import _lib

    c = gate_bwd_case(F32, 2, 3, 8, seed=8)
    cases = [(dict(dy=0), DM_ERR_ARG), (dict(z=0), DM_ERR_ARG), (dict(pre=0), DM_ERR_ARG), (dict(g=0), DM_ERR_ARG),
             (dict(dz=0), DM_ERR_ARG), (dict(batch=0), DM_ERR_ARG), (dict(seqlen=0), DM_ERR_ARG), (dict(dim=-4), DM_ERR_ARG),
             (dict(batch=32768), DM_ERR_ARG), (dict(seqlen=65536), DM_ERR_ARG), (dict(io_dtype=3), DM_ERR_DTYPE)]
    for kw, want in cases:
        m = _gbw_build(gpu, c)
        for k, v in kw.items():
            setattr(m.a, k, v)
        assert _raw("dm_gate_bwd", m.a) == want, kw
        torch.cuda.synchronize()
        assert _untouched(m.g) and _untouched(m.dz), kw
    assert int(_lib.load().dm_gate_bwd(None, None)) == DM_ERR_ARG
    _gbw_run(gpu, gate_bwd_case(F32, 32767, 1, 8, seed=9))


# =====================================================================================================================================
# dm_sum_partials
# =====================================================================================================================================
def _sp_build(gpu, c, col_off=8, extra=24):
    """out = columns col_off .. col_off + cols of a [rows, cols + extra] buffer (extra and col_off multiples of 4)."""
    from diffma_amd._lib import dm_sum_partials_args

    x = c.x.to(gpu)
    sr = c.cols + extra
    m = NS(c=c, keep=[x])
    m.obuf, m.out = _frame(gpu, c.dt, (c.rows, c.cols), (sr, 1), col_off)
    a = dm_sum_partials_args()
    a.rows, a.nw, a.cols, a.out_dtype = c.rows, c.nw, c.cols, CODE[c.dt]
    setattr(a, "in", x.data_ptr())
    a.out, a.out_sr = m.out.data_ptr(), sr
    m.a = a
    return m


def _sp_finish(m):
    torch.cuda.synchronize()
    _intact(m.obuf, m.out, "sum_partials out")
    out = m.out.cpu()
    sum_partials_eval(m.c, out)
    return out


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_sum_partials_shapes_vs_fp64(gpu, dt):
    """rows 1, 5, 37 x nw 1, 2, 7, 16 x cols 4, 32, 36, 256 (37 x 32 / 4 = 296 threads crosses a workgroup), integer and real inputs, out
    a column block of a wider buffer at column 8 (16-byte aligned) and at column 4 (a 16-bit out 8- but not 16-byte aligned)."""
    for integer in (True, False):
        for rows in (1, 5, 37):
            for nw in (1, 2, 7, 16):
                for cols in (4, 32, 36, 256):
                    c = sum_partials_case(dt, rows, nw, cols, integer, seed=rows * 100 + nw)
                    for col_off in (8, 4):
                        m = _sp_build(gpu, c, col_off)
                        _ok("dm_sum_partials", m.a)
                        _sp_finish(m)


def test_sum_partials_refusals_and_wrapper_fallback(gpu):
    from diffma_amd import _lib, hip_ops

    c = sum_partials_case(BF16, 5, 3, 8, True)

    def refused(want, col_off=8, extra=24, **kw):
        m = _sp_build(gpu, c, col_off, extra)
        for k, v in kw.items():
            setattr(m.a, k, v)
        assert _raw("dm_sum_partials", m.a) == want, (col_off, extra, kw)
        torch.cuda.synchronize()
        assert _untouched(m.out)
        return m

    refused(DM_ERR_ARG, cols=6)
    refused(DM_ERR_LAYOUT, out_sr=34)
    refused(DM_ERR_LAYOUT, col_off=2)
    m = refused(DM_ERR_DTYPE, out_dtype=5)
    refused(DM_ERR_LAYOUT, **{"in": m.keep[0].data_ptr() + 4})
    refused(DM_ERR_ARG, rows=0)
    refused(DM_ERR_ARG, nw=0)
    refused(DM_ERR_ARG, out=0)
    assert int(_lib.load().dm_sum_partials(None, None)) == DM_ERR_ARG
    # the wrapper on two refused layouts (cols % 4, a row stride that is no multiple of 4): its ATen fallback gives the right values
    for cols, sr, off in ((6, 16, 4), (8, 13, 0)):
        cw = sum_partials_case(F32, 5, 3, cols, True)
        buf = torch.full((5, sr), SENT, device=gpu)
        out = buf[:, off:off + cols]
        hip_ops.sum_partials(cw.x.to(gpu), out)
        torch.cuda.synchronize()
        sum_partials_eval(cw, out.cpu())
        assert bool((buf[:, :off] == SENT).all()) and bool((buf[:, off + cols:] == SENT).all())


# =====================================================================================================================================
# dm_colsum_f32
# =====================================================================================================================================
def _cs_build(gpu, x):
    from diffma_amd._lib import dm_colsum_args

    xd = x.to(gpu)
    m = NS(x=x, keep=[xd])
    m.obuf, m.out = _frame(gpu, F32, (x.shape[1],), (1,), 8)
    a = dm_colsum_args()
    setattr(a, "in", xd.data_ptr())
    a.out, a.rows, a.cols = m.out.data_ptr(), x.shape[0], x.shape[1]
    m.a = a
    return m


@pytest.mark.parametrize("R", COLSUM_R)
def test_colsum_rows_and_widths_vs_fp64(gpu, R):
    """Row counts around the four-in-flight loop (64) and its 16-wave tail, widths around one workgroup (256 columns) and two;
    integer input exact, real input within bound, and the same bits on a second launch."""
    for C in COLSUM_C:
        for integer in (True, False):
            m = _cs_build(gpu, colsum_case(R, C, integer, seed=R + C))
            _ok("dm_colsum_f32", m.a)
            torch.cuda.synchronize()
            _intact(m.obuf, m.out, "colsum out")
            first = m.out.cpu()
            colsum_eval(m.x, first, integer)
            m.out.fill_(NAN)
            _ok("dm_colsum_f32", m.a)
            torch.cuda.synchronize()
            assert bits_equal(m.out.cpu(), first)


def test_colsum_refusals_and_wrapper_row_classes(gpu):
    from diffma_amd import _lib, hip_ops

    x = colsum_case(5, 8, True)
    m = _cs_build(gpu, x)
    base = {k: getattr(m.a, k) for k in ("in", "out", "rows", "cols")}
    for kw, want in ((dict(cols=6), DM_ERR_ARG), (dict(rows=0), DM_ERR_ARG), (dict(cols=0), DM_ERR_ARG), (dict(out=0), DM_ERR_ARG),
                     ({"in": 0}, DM_ERR_ARG), ({"in": base["in"] + 4}, DM_ERR_LAYOUT), (dict(out=base["out"] + 8), DM_ERR_LAYOUT)):
        for k, v in {**base, **kw}.items():
            setattr(m.a, k, v)
        assert _raw("dm_colsum_f32", m.a) == want, kw
    assert int(_lib.load().dm_colsum_f32(None, None)) == DM_ERR_ARG
    torch.cuda.synchronize()
    assert _untouched(m.out)
    # hip_ops.colsum: the row-class split (R >= 256, R even, at least 16 rows per class) and its exclusions
    for R in (255, 256, 257, 272, 768):
        for C in (4, 28):
            xi = colsum_case(R, C, True)
            colsum_eval(xi, hip_ops.colsum(xi.to(gpu)).cpu(), True)


# =====================================================================================================================================
# dm_gate_head_fwd / dm_gate_head_bwd
# =====================================================================================================================================
def _gh_build(gpu, c, nblk=2, strided=False, a_off=8):
    from diffma_amd._lib import dm_gate_head_args

    sr = c.C + (16 if strided else 0)
    m = NS(c=c, nblk=nblk, keep=[])
    hbuf, h = _frame(gpu, c.dt, (c.R, c.C), (sr, 1), 8, c.h)
    w2 = c.w2.to(gpu)
    m.abuf, m.a_out = _frame(gpu, c.dt, (c.R,), (1,), a_off)
    abuf_in, a_in = _frame(gpu, c.dt, (c.R,), (1,), a_off, c.a)
    dabuf, da = _frame(gpu, c.dt, (c.R,), (1,), a_off, c.da)
    m.dhbuf, m.dh = _frame(gpu, c.dt, (c.R, c.C), (sr + 8, 1), 8)
    m.pbuf, m.part = _frame(gpu, F32, (nblk, 2 * c.C + 4), (2 * c.C + 4, 1), 4)
    m.keep += [hbuf, h, w2, abuf_in, a_in, dabuf, da]
    a = dm_gate_head_args()
    a.rows, a.C, a.io_dtype, a.nblk = c.R, c.C, CODE[c.dt], nblk
    a.h, a.h_sr, a.w2 = h.data_ptr(), sr, w2.data_ptr()
    if c.b1 is not None:
        b1 = c.b1.to(gpu)
        m.keep.append(b1)
        a.b1 = b1.data_ptr()
    if c.b2 is not None:
        b2 = c.b2.to(gpu)
        m.keep.append(b2)
        a.b2 = b2.data_ptr()
    a.a = m.a_out.data_ptr()
    m.args, m.a_in, m.da = a, a_in, da
    return m


def _gh_fwd(gpu, c, **kw):
    m = _gh_build(gpu, c, **kw)
    _ok("dm_gate_head_fwd", m.args)
    torch.cuda.synchronize()
    _intact(m.abuf, m.a_out, "gate_head a")
    gh_fwd_eval(c, m.a_out.cpu())


def _gh_bwd(gpu, c, **kw):
    m = _gh_build(gpu, c, **kw)
    a = m.args
    a.a, a.da, a.dh, a.dh_sr, a.part = m.a_in.data_ptr(), m.da.data_ptr(), m.dh.data_ptr(), m.dh.stride(0), m.part.data_ptr()
    _ok("dm_gate_head_bwd", a)
    torch.cuda.synchronize()
    _intact(m.dhbuf, m.dh, "gate_head dh")
    _intact(m.pbuf, m.part, "gate_head part")
    gh_bwd_eval(c, m.dh.cpu(), m.part.cpu(), m.nblk)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_gate_head_widths_vs_fp64(gpu, dt):
    """Rows 9, widths on both sides of every NIT step; b1 NULL; b2 NULL; h / dh as strided views; a / da one element off a 16-byte
    boundary (scalar accesses).  x = h + b1 at +-30, +-100 and around -1.278, rows with s + b2 near +-20, `a` supplied with 0 and 1."""
    for i, c in enumerate(gh_cases(dt)):
        kw = dict(strided=i % 2 == 1, a_off=8 + (i % 3 == 0))
        _gh_fwd(gpu, c, **kw)
        _gh_bwd(gpu, c, **kw)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_gate_head_fwd_grid_stride(gpu, dt):
    """rows 16389 = 4 * 4096 + 5: the 4096-workgroup cap, five rows in a second trip."""
    for C in (VECMAX[dt], 64):
        _gh_fwd(gpu, gh_case(dt, 4 * 4096 + 5, C, seed=960 + C))


@pytest.mark.parametrize("nblk,rows", GH_NBLK)
@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_gate_head_bwd_nblk_chosen_by_the_test(gpu, dt, nblk, rows):
    """One workgroup walks all 37 rows; 29 rows over 12 waves; 8 workgroups for 5 rows (six of them own none and write zero rows).
    `part` is pre-filled with NaN."""
    _gh_bwd(gpu, gh_case(dt, rows, 64, seed=950 + nblk), nblk=nblk)
    _gh_bwd(gpu, gh_case(dt, rows, 64 * VECMAX[dt] + VECMAX[dt], seed=951 + nblk), nblk=nblk, strided=True)


def test_gate_head_refusals(gpu):
    from diffma_amd import _lib

    def refused(dt, C, want, bwd_only=False, **kw):
        c = gh_case(dt, 9, C, seed=970)
        m = _gh_build(gpu, c)
        a = m.args
        a.da, a.dh, a.dh_sr, a.part = m.da.data_ptr(), m.dh.data_ptr(), m.dh.stride(0), m.part.data_ptr()
        for k, v in kw.items():
            if k.endswith("_by"):                            # a pointer moved by v bytes
                setattr(a, k[:-3], getattr(a, k[:-3]) + v)
            else:
                setattr(a, k, v)
        for name in (("dm_gate_head_bwd",) if bwd_only else ("dm_gate_head_fwd", "dm_gate_head_bwd")):
            assert _raw(name, a) == want, (name, NAME[dt], C, kw)
        torch.cuda.synchronize()
        assert _untouched(m.a_out) and _untouched(m.dh) and _untouched(m.part)

    refused(F32, 1028, DM_ERR_ARG)
    refused(BF16, 2056, DM_ERR_ARG)
    refused(F16, 2056, DM_ERR_ARG)
    refused(F32, 6, DM_ERR_ARG)
    refused(BF16, 4, DM_ERR_ARG)
    for dt in DTYPES:
        es = 4 if dt == F32 else 2
        refused(dt, 64, DM_ERR_ARG, h_sr=65)
        refused(dt, 64, DM_ERR_ARG, bwd_only=True, dh_sr=73)
        refused(dt, 64, DM_ERR_ARG, h_by=es)
        refused(dt, 64, DM_ERR_ARG, bwd_only=True, dh_by=es)
        refused(dt, 64, DM_ERR_ARG, w2_by=4)
        refused(dt, 64, DM_ERR_ARG, b1_by=4)
    refused(F32, 64, DM_ERR_ARG, bwd_only=True, nblk=0)
    refused(F32, 64, DM_ERR_ARG, rows=0)
    for k in ("h", "w2", "a"):
        refused(F32, 64, DM_ERR_ARG, **{k: 0})
    for k in ("da", "dh", "part"):
        refused(F32, 64, DM_ERR_ARG, bwd_only=True, **{k: 0})
    refused(F32, 64, DM_ERR_DTYPE, io_dtype=7)
    assert int(_lib.load().dm_gate_head_fwd(None, None)) == DM_ERR_ARG
    assert int(_lib.load().dm_gate_head_bwd(None, None)) == DM_ERR_ARG


# =====================================================================================================================================
# the dm_*_n entries of the four merge.hip operators
# =====================================================================================================================================
def _merge_pair(gpu, dt, bump2=(), n=2):
    cs = [merge_case(dt, 2, 3, 16, 2, table="perm", gated=True, want_pre=True, seed=20 + i) for i in range(n)]
    return [_merge_build(gpu, c, bump2 if i == 1 else ()) for i, c in enumerate(cs)]


def _gbw_pair(gpu, dt, bump2=(), n=2):
    return [_gbw_build(gpu, gate_bwd_case(dt, 2, 3, 16, seed=30 + i), bump2 if i == 1 else ()) for i in range(n)]


def _sp_pair(gpu, dt, bump2=(), n=2):
    return [_sp_build(gpu, sum_partials_case(dt, 5, 3, 8, i % 2 == 0, seed=40 + i), 4 if (i == 1 and bump2) else 8) for i in range(n)]


def _cs_pair(gpu, dt, bump2=(), n=2):
    return [_cs_build(gpu, colsum_case(17, 8, i % 2 == 0, seed=50 + i)) for i in range(n)]


def _cs_finish(m):
    torch.cuda.synchronize()
    _intact(m.obuf, m.out, "colsum out")
    out = m.out.cpu()
    colsum_eval(m.x, out, bool((m.x == m.x.round()).all()))
    return out


N_OPS = {"dm_token_merge": (_merge_pair, _merge_finish, "in", lambda m: (m.out, m.pre)),
         "dm_gate_bwd": (_gbw_pair, _gbw_finish, "dz", lambda m: (m.g, m.dz)),
         "dm_sum_partials": (_sp_pair, _sp_finish, "out", lambda m: (m.out,)),
         "dm_colsum_f32": (_cs_pair, _cs_finish, None, lambda m: (m.out,))}


def _flat(r):
    return [t for t in (r if isinstance(r, tuple) else (r,)) if t is not None]


@pytest.mark.parametrize("name", list(N_OPS))
def test_n_entries_pairs_singles_and_failures(gpu, name):
    """Two congruent structs (one launch), two that differ only in one pointer's 16-byte alignment (pairs_* keeps them apart), three
    structs (a pair and a single launch): every result bit for bit that of its own single call and within bound of fp64.  A second
    struct that fails its check: its status comes back, the first struct's outputs are written, the second's are untouched.
    n = 0 and null args are DM_ERR_ARG."""
    from diffma_amd import _lib

    build, finish, bump, outs = N_OPS[name]
    dts = [F32] if name == "dm_colsum_f32" else DTYPES
    for dt in dts:
        for n, bump2 in ((2, ()), (2, (bump,)), (3, ())):
            if bump2 == (None,) or (name == "dm_sum_partials" and bump2 and dt == F32):
                continue                                     # colsum and an fp32 sum_partials out have one alignment only
            singles = []
            for m in build(gpu, dt, bump2, n):
                _ok(name, m.a)
                singles.append(_flat(finish(m)))
            ms = build(gpu, dt, bump2, n)
            assert _raw_n(name, [m.a for m in ms]) == DM_OK
            for m, want in zip(ms, singles):
                got = _flat(finish(m))
                assert len(got) == len(want) and all(bits_equal(g, w) for g, w in zip(got, want)), (NAME[dt], n, bump2)
        ms = build(gpu, dt, (), 2)
        setattr(ms[1].a, "g" if name == "dm_gate_bwd" else "out", 0)
        assert _raw_n(name, [m.a for m in ms]) == DM_ERR_ARG
        finish(ms[0])
        assert all(_untouched(t) for t in outs(ms[1]))
        ms = build(gpu, dt, (), 2)
        assert _raw_n(name, [m.a for m in ms], n=0) == DM_ERR_ARG
        torch.cuda.synchronize()
        assert all(_untouched(t) for m in ms for t in outs(m))
    assert int(getattr(_lib.load(), name + "_n")(None, 2, None)) == DM_ERR_ARG


def test_zz_error_to_bound_ratios(gpu):
    """Prints the largest error-to-bound ratio per operator and dtype that the tests of this file have seen so far (run it with -s)."""
    for k in sorted(RATIOS):
        print(f"gpu ratio {k[0]:14s} {k[1]}: {RATIOS[k]:.3f}")
    assert all(v <= 1.0 for v in RATIOS.values())
