"""K8 (csrc/block_ops.hip) operator by operator against fp64: dm_ln_mod_fwd / dm_ln_mod_bwd and dm_blend_fwd / dm_blend_bwd.

Most cases go through the C ABI with hand-built argument structs, so the row strides, view offsets, rows_per_block and every
dtype combination are chosen by the test rather than by the wrappers.  The reference is plain torch fp64 autograd on the very values
the kernel reads (inputs rounded to their storage dtype first).  Every output and every gradient is compared on its own, per element.

Bounds (u = unit roundoff of the STORED dtype: 2^-8 bf16, 2^-11 fp16, 0 fp32, plus 2^-24 absolute for fp16 subnormals; eps32 = 2^-24):
  * the kernels compute in fp32.  A row reduction over C values is a per-lane sequential sum of ceil(C / 64) terms followed by a
    6-step wave tree, so its rounding error is below (ceil(C/64) + 6) * eps32 * sum|terms|.  GAM_C = 4 (ceil(C/64) + 8) eps32 covers
    that with room for the products that feed the sums and for rsqrtf (<= 2 ulp).
  * statistics: |mean - ref| <= GAM_C * mean|r|;  |rstd/ref - 1| <= GAM_C + (GAM_C * mean|r| * rstd)^2 (a mean off by d changes the
    two-pass variance by d^2 only).  A one-pass E[x^2] - mean^2 loses mean^2 * GAM_C absolutely and fails the offset rows.
  * normalised value xh: absolute error E_xh = GAM_C * S_row with S_row = 1 + max|xh| + rstd * mean|r| (the mean's error, scaled by
    rstd, plus the relative error of rstd).  Elementwise outputs: u * |ref| + propagation of E_xh through gamma and (1 + scale)
    + GAM_C times the magnitude of the terms.
  * dx = rstd (dxh - mean(dxh) - xh mean(dxh xh)), dxh = gn * gamma: every term carries E_xh or a row reduction error, so
    |err| <= u |ref| + 4 GAM_C rstd D_row S_row (1 + max|xh|), D_row = max|dxh| of the row.
  * column reductions (dshift, dscale, dgamma, dbeta, dgate): each wave sums rpb/4 rows, four waves meet in LDS, the test adds the
    partial rows in fp64: GAM_R = 2 (rpb/4 + 8) eps32 times the sum over rows of |term|, plus the sum of the terms' own E_xh error.
The bounds scale with sum|terms| rather than with |ref| because a reduction with cancellation is only as good as its terms.
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
DM_OK, DM_ERR_ARG, DM_ERR_DTYPE = 0, -1, -3
LN_PAIRS = [(F32, F32), (F32, BF16), (BF16, BF16), (F32, F16), (F16, F16)]
BLEND_TRIPLES = [(F32, F32, F32), (F32, BF16, BF16), (F32, BF16, F32), (BF16, BF16, BF16), (F32, F16, F16), (F32, F16, F32),
                 (F16, F16, F16)]


def _gam_c(C):
    return 4 * (math.ceil(C / 64) + 8) * EPS32


def _gam_r(rpb):
    return 2 * (rpb / 4 + 8) * EPS32


def _raw(name, a):
    """Status code of one C-ABI call (no exception: the argument-check cases compare it)."""
    from diffma_amd import _lib

    return int(getattr(_lib.load(), name)(ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))


def _ok(name, a):
    from diffma_amd import _lib

    rc = _raw(name, a)
    if rc != DM_OK:
        raise _lib.DiffmaHipError(f"{name} -> {rc}: {_lib.load().dm_last_error().decode()}")


def _check(name, got, ref, tol):
    """Per-element |got - ref| <= tol (NaN in got -- an element the kernel never wrote -- fails)."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{name}: {int(bad.sum())} of {ref.numel()} elements out of bound; first at flat {i}: "
                             f"got {float(got.flatten()[i])} ref {float(ref.flatten()[i])} tol {float(tol.flatten()[i])}")


def _mask_values(B, L, g):
    m = torch.rand(B, L, generator=g)
    m[:, 0] = 0.0
    if L > 1:
        m[:, 1] = 1.0
    return m


# =====================================================================================================================================
# dm_ln_mod_fwd / dm_ln_mod_bwd
# =====================================================================================================================================
def _ln_run(gpu, B, L, C1, C2=0, xdt=F32, ydt=F32, mdt=F32, affine=True, mod=True, mask=True, dy2=True, eps=1e-5, rpb=4,
            x_mode="contig", mod_view="own", dx_mode="fresh", accumulate=False, dx_add=False, xgen="randn", seed=0):
    """Build the case, run fwd and bwd through the C ABI, compare everything with fp64 autograd."""
    from diffma_amd._lib import dm_ln_mod_args

    g = torch.Generator().manual_seed(seed)
    C, R = C1 + C2, B * L
    dy2 = dy2 and mask
    # ---- host values (rounded to the storage dtypes) ------------------------------------------------------------------------
    if xgen == "offset":
        r64 = 1e3 + torch.randn(R, C, generator=g, dtype=torch.float64)
    elif xgen == "smallvar":                 # variance ~ 1e-4 next to eps = 0.1: eps in the wrong place shows
        r64 = 0.5 + 1e-2 * torch.randn(R, C, generator=g, dtype=torch.float64)
    else:
        r64 = torch.randn(R, C, generator=g, dtype=torch.float64) * 1.5 + 0.3
    if xgen == "const":                      # every third row constant: variance 0, rstd = eps^-1/2
        r64[::3] = r64[::3, :1].expand(-1, C)
    xh_ = r64[:, :C1].to(xdt)
    x2h = r64[:, C1:].to(xdt) if C2 else None
    gam = (1 + 0.5 * torch.randn(C, generator=g)).float() if affine else None
    bet = (0.5 * torch.randn(C, generator=g)).float() if affine else None
    modbuf = (0.7 * torch.randn(B, 3 * C, generator=g)).to(mdt)
    sh_h, sc_h = (modbuf[:, :C], modbuf[:, C:2 * C]) if mod else (None, None)
    mk_h = _mask_values(B, L, g).reshape(R).to(mdt) if mask else None
    dy1h = torch.randn(R, C, generator=g).to(ydt)
    dy2h = torch.randn(R, C, generator=g).to(ydt) if dy2 else None
    prior = torch.randn(R, C1, generator=g).to(xdt) if accumulate else None
    prior2 = torch.randn(R, C2, generator=g).to(xdt) if (accumulate and C2) else None
    addh = torch.randn(R, C1, generator=g).to(xdt) if dx_add else None

    # ---- device layouts ------------------------------------------------------------------------------------------------------
    if x_mode == "strided":
        xbuf = torch.full((R, C1 + 8), 9.0, dtype=xdt, device=gpu)
        xd = xbuf[:, :C1]
    elif x_mode == "offset":                 # one element off: not 16-byte aligned, the scalar instantiation
        xbuf = torch.full((R * C1 + 1,), 9.0, dtype=xdt, device=gpu)
        xd = xbuf[1:].view(R, C1)
    else:
        xd = torch.empty(R, C1, dtype=xdt, device=gpu)
    xd.copy_(xh_)
    x2d = x2h.to(gpu) if C2 else None
    gd = gam.to(gpu) if affine else None
    bd = bet.to(gpu) if affine else None
    if mod and mod_view == "chunk":          # shift / scale as the block passes them: chunks of ONE [B, 3C] adaLN output
        md = modbuf.to(gpu)
        shd, scd, msb = md[:, :C], md[:, C:2 * C], 3 * C
    elif mod:
        shd, scd, msb = sh_h.contiguous().to(gpu), sc_h.contiguous().to(gpu), C
    else:
        shd = scd = None
        msb = 0
    mkd = mk_h.to(gpu) if mask else None
    y12 = torch.full((2, R, C), float("nan"), dtype=ydt, device=gpu)
    stats = torch.full((R, 2), float("nan"), device=gpu)

    a = dm_ln_mod_args()
    a.batch, a.rows_per_batch, a.C1, a.C2 = B, L, C1, C2
    a.x_dtype, a.y_dtype, a.mod_dtype = CODE[xdt], CODE[ydt], CODE[mdt]
    a.eps = eps
    a.x, a.x2 = xd.data_ptr(), (x2d.data_ptr() if C2 else 0)
    a.gamma, a.beta = (gd.data_ptr(), bd.data_ptr()) if affine else (0, 0)
    a.shift, a.scale = (shd.data_ptr(), scd.data_ptr()) if mod else (0, 0)
    a.mask = mkd.data_ptr() if mask else 0
    a.y1, a.y2, a.stats = y12[0].data_ptr(), (y12[1].data_ptr() if mask else 0), stats.data_ptr()
    a.x_sr, a.x2_sr, a.y_sr, a.mod_sb = xd.stride(0), (C2 if C2 else 0), C, msb
    _ok("dm_ln_mod_fwd", a)

    # backward
    dy1d = dy1h.to(gpu)
    dy2d = dy2h.to(gpu) if dy2 else None
    if dx_mode == "strided":                 # dx a column block of a wider buffer: the sentinel columns must survive
        dxbuf = torch.full((R, C1 + 12), 7.0, dtype=xdt, device=gpu)
        dxd = dxbuf[:, 3:3 + C1]
    else:
        dxbuf = None
        dxd = torch.full((R, C1), float("nan"), dtype=xdt, device=gpu)
    dx2d = torch.full((R, C2), float("nan"), dtype=xdt, device=gpu) if C2 else None
    if accumulate:
        dxd.copy_(prior)
        if C2:
            dx2d.copy_(prior2)
    if dx_add:                               # its own row stride, different from dx's
        addbuf = torch.full((R, C1 + 4), 5.0, dtype=xdt, device=gpu)
        addd = addbuf[:, :C1]
        addd.copy_(addh)
        add_before = addbuf.clone()
    rpb_eff = rpb if rpb > 0 else 28
    bpb = (L + rpb_eff - 1) // rpb_eff
    part = torch.full((B * bpb, 4, C), float("nan"), device=gpu)
    a.rows_per_block = rpb
    a.dy1, a.dy2 = dy1d.data_ptr(), (dy2d.data_ptr() if dy2 else 0)
    a.dx, a.dx2, a.part = dxd.data_ptr(), (dx2d.data_ptr() if C2 else 0), part.data_ptr()
    a.dx_sr, a.dx2_sr = dxd.stride(0), (C2 if C2 else 0)
    a.accumulate = 1 if accumulate else 0
    if dx_add:
        a.dx_add, a.dxa_sr = addd.data_ptr(), addd.stride(0)
    _ok("dm_ln_mod_bwd", a)
    torch.cuda.synchronize()

    # ---- fp64 reference ------------------------------------------------------------------------------------------------------
    r = torch.cat([xh_] + ([x2h] if C2 else []), 1).double().requires_grad_(True)
    bidx = torch.arange(R) // L
    g64 = gam.double().requires_grad_(True) if affine else None
    b64 = bet.double().requires_grad_(True) if affine else None
    sh64 = sh_h.double().requires_grad_(True) if mod else None
    sc64 = sc_h.double().requires_grad_(True) if mod else None
    mk64 = mk_h.double() if mask else None
    mean = r.mean(1, keepdim=True)
    var = ((r - mean) ** 2).mean(1, keepdim=True)
    rstd = (var + eps).rsqrt()
    xhat = (r - mean) * rstd
    n = xhat * g64 + b64 if affine else xhat
    m = n * (1 + sc64[bidx]) + sh64[bidx] if mod else n
    y1 = m
    y2 = m * mk64[:, None] if mask else None
    loss = (y1 * dy1h.double()).sum() + ((y2 * dy2h.double()).sum() if dy2 else 0.0)
    wrt = [r] + ([g64, b64] if affine else []) + ([sh64, sc64] if mod else [])
    grads = torch.autograd.grad(loss, wrt)
    dr = grads[0]
    gl = dict(zip(["g", "b"], grads[1:3])) if affine else {}
    ml = dict(zip(["sh", "sc"], grads[-2:])) if mod else {}

    # ---- bounds ------------------------------------------------------------------------------------------------------------------
    with torch.no_grad():
        gc, gr = _gam_c(C), _gam_r(rpb_eff)
        absr = r.detach().abs().mean(1, keepdim=True)
        xa = xhat.detach()
        rs = rstd.detach()
        S = 1 + xa.abs().amax(1, keepdim=True) + rs * absr
        E_xh = gc * S
        ga = gam.double().abs() if affine else torch.ones(C, dtype=torch.float64)
        ba = bet.double().abs() if affine else torch.zeros(C, dtype=torch.float64)
        sca = (1 + sc_h.double()[bidx]).abs() if mod else torch.ones(1, dtype=torch.float64)
        sha = sh_h.double()[bidx].abs() if mod else torch.zeros(1, dtype=torch.float64)
        na = n.detach().abs()
        E_n = ga * E_xh + gc * (xa.abs() * ga + ba)
        E_y = E_n * sca + gc * (na * sca + sha)
        uy, ux = UNIT[ydt], UNIT[xdt]
        y1r = y1.detach()
        _check("stats.mean", stats[:, 0], mean.detach()[:, 0], (gc * absr)[:, 0])
        _check("stats.rstd", stats[:, 1], rs[:, 0], (rs * (gc + (gc * absr * rs) ** 2))[:, 0])
        _check("y1", y12[0], y1r, uy * y1r.abs() + E_y + TINY[ydt])
        if mask:
            y2r = y2.detach()
            _check("y2", y12[1], y2r, uy * y2r.abs() + E_y * mk64[:, None] + TINY[ydt])

        # backward terms
        gm = dy1h.double() + (dy2h.double() * mk64[:, None] if dy2 else 0.0)
        gn = gm * (1 + sc_h.double()[bidx]) if mod else gm
        dxh = (gn * ga).abs()
        D = dxh.amax(1, keepdim=True)
        E_dx = 4 * gc * rs * D * S * (1 + xa.abs().amax(1, keepdim=True))
        old = torch.cat([prior.double() if accumulate else torch.zeros(R, C1, dtype=torch.float64)]
                        + ([prior2.double() if accumulate else torch.zeros(R, C2, dtype=torch.float64)] if C2 else []), 1)
        if dx_add:
            old[:, :C1] += addh.double()
        dref = dr + old
        tol_dx = ux * dref.abs() + E_dx + TINY[xdt]
        _check("dx", dxd, dref[:, :C1], tol_dx[:, :C1])
        if C2:
            _check("dx2", dx2d, dref[:, C1:], tol_dx[:, C1:])
        if dx_mode == "strided":
            side = torch.cat([dxbuf[:, :3], dxbuf[:, 3 + C1:]], 1)
            assert bool((side == 7.0).all()), "dx: the kernel wrote outside the dx view"
        if dx_add:
            assert torch.equal(addbuf, add_before), "dx_add must be read-only"

        # column reductions: sum the partial rows in fp64 (the reduction the wrappers do is theirs)
        p = part.double().cpu().view(B, bpb, 4, C)
        per_b = p.sum(1)                                               # [B, 4, C]
        def colsum_b(t):                                               # sum over the rows of each batch
            return t.view(B, L, C).sum(1)
        if mod:
            _check("dshift", per_b[:, 0], ml["sh"], gr * colsum_b(gm.abs()))
            _check("dscale", per_b[:, 1], ml["sc"], gr * colsum_b((gm * na).abs()) + colsum_b(gm.abs() * ga * E_xh))
        else:
            assert bool((per_b[:, :2] == 0).all()) if not mask else True
        dg_ref = gl["g"] if affine else (gn * xa).sum(0)
        db_ref = gl["b"] if affine else gn.sum(0)
        _check("dgamma", per_b[:, 2].sum(0), dg_ref, gr * (gn * xa).abs().sum(0) + (gn.abs() * E_xh).sum(0))
        _check("dbeta", per_b[:, 3].sum(0), db_ref, gr * gn.abs().sum(0))


@pytest.mark.parametrize("mask", [True, False], ids=["mask", "nomask"])
@pytest.mark.parametrize("mdt", [F32, BF16, F16], ids=["m32", "mbf16", "mf16"])
@pytest.mark.parametrize("xdt,ydt", LN_PAIRS, ids=["f32-f32", "f32-bf16", "bf16-bf16", "f32-f16", "f16-f16"])
def test_ln_mod_dtypes_vs_fp64(gpu, xdt, ydt, mdt, mask):
    """Every (x, y) pair ln_entry accepts crossed with every modulation dtype, with and without the soft mask; a 16-byte
    (VEC 4) width with L % 4 != 0 and a scalar (VEC 1) width with a 28-row group whose last group is partial."""
    _ln_run(gpu, 2, 7, 64, xdt=xdt, ydt=ydt, mdt=mdt, mask=mask, mod_view="chunk", seed=1)
    _ln_run(gpu, 1, 29, 198, xdt=xdt, ydt=ydt, mdt=mdt, mask=mask, rpb=28, seed=2)


@pytest.mark.parametrize("xdt,ydt", LN_PAIRS, ids=["f32-f32", "f32-bf16", "bf16-bf16", "f32-f16", "f16-f16"])
def test_ln_mod_unmodulated_forms_vs_fp64(gpu, xdt, ydt):
    """The no_mod_t instantiation (no shift / scale, no mask, no dy2): plain LN with and without gamma / beta, and LN(cat[x, x2])
    in the 16-byte form (C1 = C2 = 64) and the scalar one (C1 = 6: 16-byte loads would straddle x | x2)."""
    _ln_run(gpu, 2, 7, 64, xdt=xdt, ydt=ydt, mod=False, mask=False, seed=3)
    _ln_run(gpu, 2, 5, 64, xdt=xdt, ydt=ydt, mod=False, mask=False, affine=False, seed=4)
    _ln_run(gpu, 2, 7, 64, 64, xdt=xdt, ydt=ydt, mod=False, mask=False, seed=5)
    _ln_run(gpu, 1, 9, 6, 10, xdt=xdt, ydt=ydt, mod=False, mask=False, seed=6)


@pytest.mark.parametrize("mdt", [F32, BF16, F16], ids=["m32", "mbf16", "mf16"])
def test_ln_mod_mask_forms_vs_fp64(gpu, mdt):
    """A mask without modulation (MOD instantiation, shift / scale NULL), and the MOD instantiation with dy2 = NULL (only y1
    receives a gradient), each with and without the mask."""
    _ln_run(gpu, 2, 7, 64, mdt=mdt, mod=False, mask=True, seed=7)
    _ln_run(gpu, 2, 7, 198, ydt=BF16, mdt=mdt, mod=False, mask=True, seed=8)
    _ln_run(gpu, 2, 7, 64, mdt=mdt, mod=True, mask=True, dy2=False, seed=9)
    _ln_run(gpu, 2, 7, 64, mdt=mdt, mod=True, mask=False, seed=10)


@pytest.mark.parametrize("C1,C2", [(1, 0), (4, 0), (64, 0), (198, 0), (512, 0), (1023, 0), (1024, 0), (6, 10), (512, 512), (300, 212)])
def test_ln_mod_widths_vs_fp64(gpu, C1, C2):
    """Every NIT of both instantiations: VEC 4 with NIT 1 / 2 / 4 (C = 4, 64, 512, 1024), VEC 1 up to NIT 16 (198, 1023, the cat
    with C1 % 4 != 0), C = 1 (variance 0, dx = 0).  Modulated + masked, and the model's autocast form (x fp32, y / mod bf16)."""
    mod = C2 == 0
    _ln_run(gpu, 2, 7, C1, C2, mod=mod, mask=mod, seed=11)
    _ln_run(gpu, 2, 5, C1, C2, ydt=BF16, mdt=BF16, mod=mod, mask=mod, rpb=8, mod_view="chunk" if mod else "own", seed=12)


@pytest.mark.parametrize("L,rpb", [(1, 4), (1, 0), (7, 4), (7, 8), (29, 28), (29, 0), (196, 28), (196, 4), (196, 8)])
def test_ln_mod_row_groups_vs_fp64(gpu, L, rpb):
    """rows_per_block 0 (= 28), 4, 8, 28 with L = 1 and L not a multiple of the group: the last group of every batch is partial."""
    _ln_run(gpu, 3, L, 64, rpb=rpb, mod_view="chunk", seed=13 + L)
    _ln_run(gpu, 2, L, 198, 0, xdt=F32, ydt=F16, mdt=F16, rpb=rpb, seed=14 + L)


@pytest.mark.parametrize("C", [64, 198])
def test_ln_mod_layouts_vs_fp64(gpu, C):
    """x as a row-strided view and as a view one element off (scalar path), shift / scale as chunks of one [B, 3C] tensor, dx a
    column block of a wider sentinel-filled buffer (the sentinel columns come back unchanged)."""
    _ln_run(gpu, 2, 7, C, x_mode="strided", mod_view="chunk", dx_mode="strided", seed=20)
    _ln_run(gpu, 2, 7, C, x_mode="offset", mod_view="chunk", dx_mode="strided", seed=21)
    _ln_run(gpu, 2, 7, C, xdt=BF16, ydt=BF16, mdt=BF16, x_mode="offset", dx_mode="strided", seed=22)


@pytest.mark.parametrize("C1,C2", [(64, 64), (6, 10), (99, 99)])
@pytest.mark.parametrize("xdt", [F32, BF16])
def test_ln_mod_bwd_accumulate_cat_vs_fp64(gpu, C1, C2, xdt):
    """accumulate = 1 in the cat form: dx / dx2 = computed + what they held (the blend's fresh gradients), both instantiations."""
    _ln_run(gpu, 2, 7, C1, C2, xdt=xdt, ydt=xdt, mod=False, mask=False, accumulate=True, seed=30)


@pytest.mark.parametrize("C,x_mode", [(64, "contig"), (64, "offset"), (198, "contig")])
@pytest.mark.parametrize("xdt", [F32, F16])
def test_ln_mod_bwd_dx_add_vs_fp64(gpu, C, x_mode, xdt):
    """dx_add (single-input form, own row stride): dx = computed + dx_add, and dx_add is bitwise unchanged (it may be shared)."""
    _ln_run(gpu, 2, 7, C, xdt=xdt, ydt=xdt, mdt=xdt, x_mode=x_mode, dx_add=True, seed=31)


@pytest.mark.parametrize("case", ["offset", "const", "eps_large", "eps_small"])
def test_ln_mod_numerics_vs_fp64(gpu, case):
    """Rows at a large common offset (1e3 + N(0, 1), fp32: a one-pass variance keeps nothing of them), constant rows (variance 0,
    rstd = eps^-1/2), eps 1e-5 and eps 0.1 next to a variance ~1e-4 (eps outside the root or added to the std is far off)."""
    if case == "offset":
        for C in (512, 1024, 198):
            _ln_run(gpu, 2, 7, C, xgen="offset", seed=40 + C)
    elif case == "const":
        _ln_run(gpu, 2, 9, 512, xgen="const", seed=41)
        _ln_run(gpu, 2, 9, 198, xgen="const", ydt=BF16, mdt=BF16, seed=42)
    elif case == "eps_large":
        _ln_run(gpu, 2, 7, 64, xgen="smallvar", eps=0.1, seed=43)
        _ln_run(gpu, 2, 7, 198, xgen="smallvar", eps=0.1, mod=False, mask=False, seed=44)
    else:
        _ln_run(gpu, 2, 7, 64, xgen="smallvar", eps=1e-5, seed=45)


def test_ln_mod_argument_checks(gpu):
    """Host-side rejections (nothing is launched): C = 1025 (more than 16 values per lane), rows_per_block 6, dx_add with x2,
    an unsupported (x, y) pair, an unsupported modulation dtype."""
    from diffma_amd._lib import dm_ln_mod_args

    B, L = 1, 4
    buf = torch.zeros(B * L * 2100, device=gpu)
    part = torch.zeros(64 * 4 * 2100, device=gpu)

    def args(C1, C2=0, **kw):
        a = dm_ln_mod_args()
        a.batch, a.rows_per_batch, a.C1, a.C2 = B, L, C1, C2
        a.x_dtype = a.y_dtype = a.mod_dtype = 0
        a.eps = 1e-5
        a.x = buf.data_ptr()
        a.x2 = buf.data_ptr() if C2 else 0
        a.y1 = a.dy1 = a.dx = buf.data_ptr()
        a.dx2 = buf.data_ptr() if C2 else 0
        a.stats = a.part = part.data_ptr()
        a.x_sr = C1
        a.x2_sr = C2
        a.y_sr = a.dx_sr = C1 + C2
        a.dx2_sr = C2
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert _raw("dm_ln_mod_fwd", args(1025)) == DM_ERR_ARG
    assert _raw("dm_ln_mod_bwd", args(1025)) == DM_ERR_ARG
    assert _raw("dm_ln_mod_bwd", args(512, 513)) == DM_ERR_ARG
    assert _raw("dm_ln_mod_bwd", args(64, rows_per_block=6)) == DM_ERR_ARG
    assert _raw("dm_ln_mod_bwd", args(32, 32, dx_add=buf.data_ptr(), dxa_sr=32)) == DM_ERR_ARG
    for xd, yd in ((1, 0), (2, 0), (1, 2), (2, 1), (0, 3)):
        assert _raw("dm_ln_mod_fwd", args(64, x_dtype=xd, y_dtype=yd)) == DM_ERR_DTYPE
        assert _raw("dm_ln_mod_bwd", args(64, x_dtype=xd, y_dtype=yd)) == DM_ERR_DTYPE
    assert _raw("dm_ln_mod_fwd", args(64, mod_dtype=5)) == DM_ERR_DTYPE
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0 and float(part.abs().sum()) == 0.0


# ---- through the wrappers: the automatic row groups and the partial-row sums ------------------------------------------------------
@pytest.mark.parametrize("small_rows", [None, 0])
def test_ln_mod_wrappers_row_groups_vs_fp64(gpu, monkeypatch, small_rows):
    """hip_ops.ln_mod_fwd / ln_mod_bwd as the block calls them (x fp32, y / mod bf16, shift / scale chunks of [B, 3C]): B = 40,
    L = 196 is above the switch (_ln_rows_per_block picks 28 by itself); a small launch with LN_SMALL_ROWS = 0 is forced to 28.
    dshift / dscale are summed by the wrapper INTO bf16: each fp32 partial row is rounded to bf16 before the sum and the sum once
    more, so on top of the module bounds they get 2^-8 (sum over groups |partial| + |ref|) <= 2^-7 sum over rows |term|."""
    from diffma_amd import hip_ops

    if small_rows is None:
        B, L = 40, 196
    else:
        monkeypatch.setattr(hip_ops, "LN_SMALL_ROWS", small_rows)
        B, L = 2, 29
    assert hip_ops._ln_rows_per_block(B, L) == 28
    C, eps = 512, 1e-5
    g = torch.Generator().manual_seed(50)
    x = torch.randn(B, L, C, generator=g) + 0.2
    gam, bet = 1 + 0.5 * torch.randn(C, generator=g), 0.5 * torch.randn(C, generator=g)
    mod = (0.7 * torch.randn(B, 3 * C, generator=g)).to(BF16)
    mk = _mask_values(B, L, g).to(BF16)
    dy1, dy2 = torch.randn(B, L, C, generator=g).to(BF16), torch.randn(B, L, C, generator=g).to(BF16)
    d = lambda t: t.to(gpu)
    md = d(mod)
    y1, y2, st = hip_ops.ln_mod_fwd(d(x), None, d(gam), d(bet), md[:, :C], md[:, C:2 * C], d(mk), eps, BF16)
    dx, _, dsh, dsc, dg, db = hip_ops.ln_mod_bwd(d(x), None, d(gam), d(bet), md[:, :C], md[:, C:2 * C], d(mk), eps, st, d(dy1),
                                                  d(dy2), mod_dtype=BF16)
    torch.cuda.synchronize()
    assert dsh.dtype == dsc.dtype == BF16
    r = x.double().requires_grad_(True)
    g64, b64 = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    sh, sc = mod[:, :C].double().requires_grad_(True), mod[:, C:2 * C].double().requires_grad_(True)
    mean = r.mean(-1, keepdim=True)
    rstd = (((r - mean) ** 2).mean(-1, keepdim=True) + eps).rsqrt()
    xh = (r - mean) * rstd
    n = xh * g64 + b64
    m = n * (1 + sc[:, None]) + sh[:, None]
    mkd = mk.double()[..., None]
    loss = (m * dy1.double()).sum() + (m * mkd * dy2.double()).sum()
    dr, rg, rb, rsh, rsc = torch.autograd.grad(loss, (r, g64, b64, sh, sc))
    with torch.no_grad():
        gc, gr = _gam_c(C), _gam_r(28)
        xa, na, mm, rs = xh.detach(), n.detach(), m.detach(), rstd.detach()
        S = 1 + xa.abs().amax(-1, keepdim=True) + rs * r.detach().abs().mean(-1, keepdim=True)
        E_xh = gc * S
        ga, sca = gam.double().abs(), (1 + sc.detach()[:, None]).abs()
        E_y = (ga * E_xh + gc * (xa.abs() * ga + bet.double().abs())) * sca + gc * (na * sca + sh.detach()[:, None].abs())
        _check("y1", y1, mm, 2.0 ** -8 * mm.abs() + E_y)
        _check("y2", y2, mm * mkd, 2.0 ** -8 * (mm * mkd).abs() + E_y * mkd)
        gm = dy1.double() + dy2.double() * mkd
        gn = gm * sca
        D = (gn * ga).abs().amax(-1, keepdim=True)
        _check("dx", dx, dr, 4 * gc * rs * D * S * (1 + xa.abs().amax(-1, keepdim=True)))
        t_sh = gm.abs().sum(1)
        _check("dshift", dsh, rsh, (2.0 ** -7 + gr) * t_sh)
        t_sc = (gm * na).abs().sum(1)
        _check("dscale", dsc, rsc, (2.0 ** -7 + gr) * t_sc + (gm.abs() * ga * E_xh).sum(1))
        # dgamma / dbeta: B * bpb fp32 partial rows summed by torch in fp32 -- eps32 per level of its reduction tree on top
        gr2 = gr + 32 * EPS32
        _check("dgamma", dg, rg, gr2 * (gn * xa).abs().sum((0, 1)) + (gn.abs() * E_xh).sum((0, 1)))
        _check("dbeta", db, rb, gr2 * gn.abs().sum((0, 1)))


@pytest.mark.parametrize("amp", [None, BF16], ids=["fp32", "bf16"])
def test_ln_autograd_passthrough_vs_fp64(gpu, amp):
    """block_ops.ln_modulate_mask and block_ops.ln_cat with passthrough=True, driven by torch.autograd.grad: the aliases' gradients
    reach the kernel as dx_add (residual, read only) and as accumulate (the two cat inputs), and every leaf gradient matches the
    fp64 gradient of the two-consumer graph (LN branch + a direct use of x, xs, ws).  Bounds: the outputs of y dtype are within
    2^-8 / fp32 rounding of the rows; the leaf gradients per element within 1e-3 (bf16: 2^-6) of their max |ref|."""
    from diffma_amd import block_ops

    B, L, C = 2, 9, 64
    dt = amp or F32
    g = torch.Generator().manual_seed(60)
    x0 = torch.randn(B, L, C, generator=g) + 0.1
    mod0 = (0.5 * torch.randn(B, 3 * C, generator=g)).to(dt)
    w0 = _mask_values(B, L, g)[..., None]
    norm = torch.nn.LayerNorm(C).to(gpu)
    with torch.no_grad():
        norm.weight.copy_(1 + 0.3 * torch.randn(C, generator=g))
        norm.bias.copy_(0.3 * torch.randn(C, generator=g))
    norm2 = torch.nn.LayerNorm(2 * C).to(gpu)
    with torch.no_grad():
        norm2.weight.copy_(1 + 0.3 * torch.randn(2 * C, generator=g))
        norm2.bias.copy_(0.3 * torch.randn(2 * C, generator=g))
    xs0, ws0 = torch.randn(B, L, C, generator=g).to(dt), torch.randn(B, L, C, generator=g).to(dt)
    d1, d2, dr = (torch.randn(B, L, C, generator=g).to(dt) for _ in range(3))
    dh, e1, e2 = torch.randn(B, L, 2 * C, generator=g).to(dt), torch.randn(B, L, C, generator=g).to(dt), torch.randn(B, L, C, generator=g).to(dt)

    # ---- device, through the autograd functions --------------------------------------------------------------------------------
    x = x0.to(gpu).requires_grad_(True)
    mod = mod0.to(gpu).requires_grad_(True)
    w = w0.to(gpu)
    xs, ws = xs0.to(gpu).requires_grad_(True), ws0.to(gpu).requires_grad_(True)
    block_ops.set_output_dtype(dt)
    block_ops.drop_mask_cache()
    shift, scale, _ = mod.chunk(3, dim=1)
    x_ssm, w_ssm, x_res = block_ops.ln_modulate_mask(x, norm, shift, scale, w, passthrough=True)
    hcat, xs_a, ws_a = block_ops.ln_cat(xs, ws, norm2, passthrough=True)
    loss = ((x_ssm.float() * d1.to(gpu).float()).sum() + (w_ssm.float() * d2.to(gpu).float()).sum() + (x_res * dr.to(gpu).float()).sum()
            + (hcat.float() * dh.to(gpu).float()).sum() + (xs_a.float() * e1.to(gpu).float()).sum() + (ws_a.float() * e2.to(gpu).float()).sum())
    leaves = (x, mod, norm.weight, norm.bias, xs, ws, norm2.weight, norm2.bias)
    got = torch.autograd.grad(loss, leaves)
    block_ops.set_output_dtype(F32)

    # ---- fp64 reference of the same graph ----------------------------------------------------------------------------------------
    X = x0.double().requires_grad_(True)
    M = mod0.double().requires_grad_(True)
    W1, B1 = norm.weight.detach().cpu().double().requires_grad_(True), norm.bias.detach().cpu().double().requires_grad_(True)
    XS, WS = xs0.double().requires_grad_(True), ws0.double().requires_grad_(True)
    W2, B2 = norm2.weight.detach().cpu().double().requires_grad_(True), norm2.bias.detach().cpu().double().requires_grad_(True)
    sh, sc, _ = M.chunk(3, dim=1)
    mm = torch.nn.functional.layer_norm(X, (C,), W1, B1, norm.eps) * (1 + sc[:, None]) + sh[:, None]
    mk = w0.to(dt).double()
    hc = torch.nn.functional.layer_norm(torch.cat([XS, WS], -1), (2 * C,), W2, B2, norm2.eps)
    ref_loss = ((mm * d1.double()).sum() + (mm * mk * d2.double()).sum() + (X * dr.double()).sum() + (hc * dh.double()).sum()
                + (XS * e1.double()).sum() + (WS * e2.double()).sum())
    refs = torch.autograd.grad(ref_loss, (X, M, W1, B1, XS, WS, W2, B2))
    rel = 2.0 ** -6 if amp else 1e-3
    names = ("x", "adaLN(shift|scale|gate)", "norm1.weight", "norm1.bias", "xs", "ws", "norm2.weight", "norm2.bias")
    for name, a_, r_ in zip(names, got, refs):
        _check(name, a_.float(), r_, rel * float(r_.abs().max()) + 0 * r_)
    u = 2.0 ** -8 if amp else 1e-5
    _check("x_ssm", x_ssm.float(), mm.detach(), u * mm.detach().abs() + 1e-5 * (1 + mm.detach().abs()))
    _check("w_ssm", w_ssm.float(), (mm * mk).detach(), u * (mm * mk).detach().abs() + 1e-5 * (1 + mm.detach().abs()))
    _check("hcat", hcat.float(), hc.detach(), u * hc.detach().abs() + 1e-5 * (1 + hc.detach().abs()))
    assert torch.equal(x_res, x) and torch.equal(xs_a, xs) and torch.equal(ws_a, ws)


# =====================================================================================================================================
# dm_blend_fwd / dm_blend_bwd
# =====================================================================================================================================
def _blend_run(gpu, B, L, C, xdt=F32, sdt=F32, gdt=F32, rpb=4, gate_mode="chunk", seed=0):
    """out = x + gate[b] * (a xs + (1 - a) ws) and its backward through the C ABI against fp64; `a` holds exact 0 and 1.
    Bounds: out u_x |ref| + 8 eps32 (|x| + |gate| (|a xs| + |(1-a) ws|)); dxs / dws u_s |ref| + 8 eps32 |ref| (one product);
    da (a row reduction over C) u_s |ref| + GAM_C sum_c |g gate (xs - ws)|; dgate partial rows (summed here in fp64) GAM_R times
    sum over rows |g (a xs + (1-a) ws)|."""
    from diffma_amd._lib import dm_blend_args

    g = torch.Generator().manual_seed(seed)
    R = B * L
    xh = torch.randn(R, C, generator=g).to(xdt)
    s1h, s2h = torch.randn(R, C, generator=g).to(sdt), torch.randn(R, C, generator=g).to(sdt)
    ah = _mask_values(B, L, g).reshape(R).to(sdt)
    gbuf = (1 + 0.5 * torch.randn(B, 3 * C, generator=g)).to(gdt)
    gh = gbuf[:, 2 * C:]
    gvh = torch.randn(R, C, generator=g).to(xdt)
    dev = lambda t: t.to(gpu)
    xd, s1d, s2d, ad, gvd = dev(xh), dev(s1h), dev(s2h), dev(ah), dev(gvh)
    if gate_mode == "chunk":                 # the third chunk of the adaLN output, row stride 3C
        gd_ = dev(gbuf)[:, 2 * C:]
        gsb = 3 * C
    else:                                    # one element off: the scalar instantiation
        gflat = torch.zeros(B * C + 1, dtype=gdt, device=gpu)
        gd_ = gflat[1:].view(B, C)
        gd_.copy_(gh)
        gsb = C
    out = torch.full((R, C), float("nan"), dtype=xdt, device=gpu)
    a = dm_blend_args()
    a.batch, a.rows_per_batch, a.C = B, L, C
    a.x_dtype, a.s_dtype, a.g_dtype = CODE[xdt], CODE[sdt], CODE[gdt]
    a.x, a.xs, a.ws, a.a, a.gate, a.out = xd.data_ptr(), s1d.data_ptr(), s2d.data_ptr(), ad.data_ptr(), gd_.data_ptr(), out.data_ptr()
    a.gate_sb = gsb
    _ok("dm_blend_fwd", a)
    rpb_eff = rpb if rpb > 0 else 28
    bpb = (L + rpb_eff - 1) // rpb_eff
    dxs = torch.full((R, C), float("nan"), dtype=sdt, device=gpu)
    dws = torch.full((R, C), float("nan"), dtype=sdt, device=gpu)
    da = torch.full((R,), float("nan"), dtype=sdt, device=gpu)
    part = torch.full((B * bpb, C), float("nan"), device=gpu)
    a.rows_per_block = rpb
    a.g, a.dxs, a.dws, a.da, a.dgate_part = gvd.data_ptr(), dxs.data_ptr(), dws.data_ptr(), da.data_ptr(), part.data_ptr()
    _ok("dm_blend_bwd", a)
    torch.cuda.synchronize()

    bidx = torch.arange(R) // L
    X, S1, S2, A = xh.double(), s1h.double().requires_grad_(True), s2h.double().requires_grad_(True), ah.double().requires_grad_(True)
    G = gh.double().requires_grad_(True)
    o = X + G[bidx] * (A[:, None] * S1 + (1 - A[:, None]) * S2)
    dS1, dS2, dA, dG = torch.autograd.grad((o * gvh.double()).sum(), (S1, S2, A, G))
    with torch.no_grad():
        ux, us = UNIT[xdt], UNIT[sdt]
        ga = G[bidx].abs()
        mix_abs = (A[:, None] * S1).abs() + ((1 - A[:, None]) * S2).abs()
        _check("out", out, o, ux * o.abs() + 8 * EPS32 * (X.abs() + ga * mix_abs) + TINY[xdt])
        _check("dxs", dxs, dS1, (us + 8 * EPS32) * dS1.abs() + TINY[sdt])
        _check("dws", dws, dS2, (us + 8 * EPS32) * dS2.abs() + TINY[sdt])
        gg = gvh.double() * G[bidx]
        _check("da", da, dA, us * dA.abs() + _gam_c(C) * (gg * (S1 - S2)).abs().sum(1) + TINY[sdt])
        dgp = part.double().cpu().view(B, bpb, C).sum(1)
        _check("dgate", dgp, dG, _gam_r(rpb_eff) * (gvh.double().abs() * mix_abs).view(B, L, C).sum(1))


@pytest.mark.parametrize("xdt,sdt,gdt", BLEND_TRIPLES, ids=["000", "011", "010", "111", "022", "020", "222"])
def test_blend_dtypes_vs_fp64(gpu, xdt, sdt, gdt):
    """All seven dtype triples blend_entry accepts, on the 16-byte path (gate = third chunk of [B, 3C]) and on the scalar path
    (gate one element off), with a partial last row group."""
    _blend_run(gpu, 2, 7, 64, xdt, sdt, gdt, seed=70)
    _blend_run(gpu, 2, 7, 64, xdt, sdt, gdt, gate_mode="offset", seed=71)


@pytest.mark.parametrize("C", [4, 198, 512, 1024])
def test_blend_widths_vs_fp64(gpu, C):
    """VEC 4 with NIT 1 / 2 / 4 and VEC 1 (C = 198) in fp32 and in the bf16 autocast triple."""
    _blend_run(gpu, 2, 7, C, seed=72)
    _blend_run(gpu, 2, 9, C, F32, BF16, BF16, rpb=8, seed=73)


@pytest.mark.parametrize("L,rpb", [(1, 4), (1, 0), (7, 4), (29, 28), (29, 0), (196, 28), (196, 8)])
def test_blend_row_groups_vs_fp64(gpu, L, rpb):
    """rows_per_block 0 (= 28), 4, 8, 28 with L = 1 and partial last groups."""
    _blend_run(gpu, 3, L, 64, rpb=rpb, seed=74 + L)
    _blend_run(gpu, 2, L, 198, F32, F16, F16, rpb=rpb, seed=75 + L)


def test_blend_argument_checks(gpu):
    """An unsupported dtype triple is DM_ERR_DTYPE, a row of 1025 values and rows_per_block 6 are DM_ERR_ARG (nothing launched)."""
    from diffma_amd._lib import dm_blend_args

    buf = torch.zeros(4 * 2100, device=gpu)

    def args(C, key=(0, 0, 0), rpb=0):
        a = dm_blend_args()
        a.batch, a.rows_per_batch, a.C = 1, 4, C
        a.x_dtype, a.s_dtype, a.g_dtype = key
        a.rows_per_block = rpb
        a.x = a.xs = a.ws = a.a = a.gate = a.out = a.g = a.dxs = a.dws = a.da = a.dgate_part = buf.data_ptr()
        a.gate_sb = C
        return a

    for key in ((0, 1, 2), (1, 0, 0), (2, 2, 0), (1, 1, 0), (0, 0, 1)):
        assert _raw("dm_blend_fwd", args(64, key)) == DM_ERR_DTYPE
        assert _raw("dm_blend_bwd", args(64, key)) == DM_ERR_DTYPE
    assert _raw("dm_blend_fwd", args(1025)) == DM_ERR_ARG
    assert _raw("dm_blend_bwd", args(1025)) == DM_ERR_ARG
    assert _raw("dm_blend_bwd", args(64, rpb=6)) == DM_ERR_ARG
    torch.cuda.synchronize()
    assert float(buf.abs().sum()) == 0.0


def test_blend_wrappers_above_the_switch_vs_fp64(gpu):
    """hip_ops.blend_fwd / blend_bwd at B = 40, L = 196, C = 512 (28-row groups chosen by _ln_rows_per_block) in the bf16 autocast
    triple.  dgate is summed by the wrapper into bf16: each partial row rounded to bf16 and the sum once more, so its bound is
    2^-8 (sum over groups |partial| + |ref|) <= 2^-7 sum over rows |term|, plus GAM_R of that sum."""
    from diffma_amd import hip_ops

    B, L, C = 40, 196, 512
    assert hip_ops._ln_rows_per_block(B, L) == 28
    g = torch.Generator().manual_seed(80)
    x = torch.randn(B, L, C, generator=g)
    xs, ws = torch.randn(B, L, C, generator=g).to(BF16), torch.randn(B, L, C, generator=g).to(BF16)
    a_row = _mask_values(B, L, g)[..., None].to(BF16)
    gbuf = (1 + 0.5 * torch.randn(B, 3 * C, generator=g)).to(BF16)
    gv = torch.randn(B, L, C, generator=g)
    d = lambda t: t.to(gpu)
    gate = d(gbuf)[:, 2 * C:]
    out = hip_ops.blend_fwd(d(x), d(xs), d(ws), d(a_row), gate)
    dxs, dws, da, dgate = hip_ops.blend_bwd(d(gv), d(xs), d(ws), d(a_row), gate)
    torch.cuda.synchronize()
    S1, S2, A, G = (t.double().requires_grad_(True) for t in (xs, ws, a_row, gbuf[:, 2 * C:]))
    o = x.double() + G[:, None] * (A * S1 + (1 - A) * S2)
    rS1, rS2, rA, rG = torch.autograd.grad((o * gv.double()).sum(), (S1, S2, A, G))
    with torch.no_grad():
        mix = (A * S1).abs() + ((1 - A) * S2).abs()
        _check("out", out, o, 8 * EPS32 * (x.double().abs() + G[:, None].abs() * mix))
        _check("dxs", dxs, rS1, 2.0 ** -8 * rS1.abs())
        _check("dws", dws, rS2, 2.0 ** -8 * rS2.abs())
        gg = gv.double() * G[:, None]
        _check("da", da, rA, 2.0 ** -8 * rA.abs() + _gam_c(C) * (gg * (S1 - S2)).abs().sum(-1, keepdim=True))
        tsum = (gv.double().abs() * mix).sum(1)
        _check("dgate", dgate, rG, (2.0 ** -7 + _gam_r(28)) * tsum)


# =====================================================================================================================================
# the soft-mask copy that feeds K8 (block_ops._mask_once)
# =====================================================================================================================================
def test_mask_cache_capture_version_and_invalidate(gpu, monkeypatch):
    """block_ops._mask_once is keyed on the mask object, its _version, step_prep's generation and the capture state:
    two captured forwards with the same `w` get copies with different storage (each lives in its own graph's pool), an eager forward
    after a capture does not get a captured copy, an in-place edit of `w` gives a fresh copy with the new values, and
    step_prep.invalidate() drops the cached copy.  Under bf16 autocast, where the mask is cast to the modulation dtype (the
    training and sampling configuration); without autocast the fp32 mask is `w` itself, reshaped, and no copy exists."""
    import numpy as np
    import os

    from diffma_amd import block_ops, step_prep
    from diffma_amd.graphed import _capture_mode
    from diffma_amd.model import DiffMa

    G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    gz = np.load(os.path.join(G, "g5_tiny_diffma.npz"))
    sd = {k[3:]: torch.from_numpy(gz[k]) for k in gz.files if k.startswith("sd.")}
    net = DiffMa(input_size=8, patch_size=2, strip_size=2, hidden_size=64, depth=4, d_state=16)
    net.load_state_dict(sd)
    net = net.to(gpu).eval()
    inp = {k: torch.from_numpy(gz[k]).to(gpu) for k in ("x", "t", "y", "y2", "w")}
    w = inp["w"]

    seen = []
    orig = block_ops._mask_once

    def spy(w_, B, L, dtype):
        m = orig(w_, B, L, dtype)
        seen.append(m)
        return m

    monkeypatch.setattr(block_ops, "_mask_once", spy)

    def fwd(amp=BF16):
        seen.clear()
        with torch.no_grad(), torch.autocast("cuda", dtype=amp, enabled=amp is not None):
            out = net(inp["x"], inp["t"], y=inp["y"], y2=inp["y2"], w=w)
        assert seen and all(m is seen[0] for m in seen), "one mask copy per forward, shared by the blocks"
        assert seen[0].dtype == (amp or F32)
        return seen[0], out

    block_ops.drop_mask_cache()
    m32, _ = fwd(None)
    assert m32.data_ptr() == w.data_ptr()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            fwd()
    torch.cuda.current_stream().wait_stream(side)
    graphs, caps = [], []
    for _ in range(2):
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, capture_error_mode=_capture_mode(gpu)):
            m, _ = fwd()
        graphs.append(gr)
        caps.append(m)
    assert caps[0].data_ptr() != caps[1].data_ptr()
    e1, _ = fwd()
    assert all(e1.data_ptr() != c.data_ptr() for c in caps) and e1 is not caps[1]
    e2, _ = fwd()
    assert e2 is e1                                              # eager, unchanged: the cached copy
    with torch.no_grad():
        w.mul_(0.5)                                              # bumps w._version
    e3, _ = fwd()
    assert e3 is not e1 and torch.equal(e3, w.reshape(e3.shape).to(e3.dtype))
    step_prep.invalidate()
    e4, _ = fwd()
    assert e4 is not e3 and torch.equal(e4, e3)
    for gr in graphs:
        gr.replay()
    torch.cuda.synchronize()
    block_ops.drop_mask_cache()
