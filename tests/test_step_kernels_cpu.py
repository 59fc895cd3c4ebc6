"""The kernels that wrap the denoiser in a training step or a sampler step (csrc/diffusion_loss.hip, csrc/diffusion_step.hip,
csrc/optim.hip): the parts that need no GPU.

Builders, fp64 references, fp32 emulations, bound functions and their self-tests for dm_q_sample, dm_training_loss,
dm_training_loss_bwd, dm_diffusion_step, dm_adamw_ema_step and dm_grads_nonfinite.  tests/test_step_kernels_gpu.py imports all of it and
feeds the kernels' outputs to the same `*_eval` functions the emulations go through here.

Tables.  `schedule(spec)` takes the fp64 host arrays of create_diffusion(spec) ("" = 1000 steps, "250"), rounds them to fp32 (fp32
tables are the ABI's contract) and stacks them in a PERMUTED order into an array of NROWS rows, four more than any kernel needs; the
spare rows are NaN, so a kernel that reads a wrong row_* fails on every element.

References.  The operation in fp64 on exactly the fp32 / 16-bit values the kernel receives.  Each operator is written ONCE (`*_math`)
with the working dtype as a parameter: fp64 gives the reference, fp32 -- torch rounds after every operation, nothing is contracted --
gives the emulation in the kernel's order of operations.  dm_training_loss rounds (v + 1) and (1 - frac) to the model output's dtype in
BOTH (diffusion_loss.hip:80-83, the reference project's expression; for an fp32 output that is a rounding to fp32); dm_diffusion_step
rounds neither (include/diffma_hip.h).  AdamW + EMA follow the header's formulas in fp64 from the fp32 state, the double hyper-parameters
unrounded.

Bounds.  E = 2^-24.  A correctly rounded fp32 operation errs by at most E |result|; expf, logf and tanhf are charged 2 ulp = 4 E |result|;
sqrtf and the division are correctly rounded in this build (hipcc's default) and are charged E, except inside AdamW where they are charged
2 E.  a b + c d costs 2 E (|a b| + |c d|): two products and a sum (an FMA only removes roundings).  d_x below is the bound carried by x.
  * q_sample: 2 E (|sqrt_ac x0| + |sqrt_1mac noise|).
  * training_loss, per element.  frac and omf = rnd(1 - frac) are exact (see above).
      d_lv = 2 E (|frac maxl| + |omf minl|);  d_px0 = 2 E (|sr xt| + |srm1 eps|);  d_mean = |c1| d_px0 + 2 E (|c1 px0| + |c2 xt|);
      d_tmean = 2 E (|c1 x0| + |c2 xt|).
      grad eps half = -2 (nz - eps) inv_n: 3 E |ref| (the difference, inv_n, the product).
      KL (t > 0): diff = tmean - mean, d_diff = d_mean + d_tmean + E |diff|;  dd = minl - lv, d_dd = d_lv + E |dd|;
        ed = expf(dd), d_ed = ed (d_dd + 4 E);  el = expf(-lv), d_el = el (d_lv + 4 E);
        q = diff^2 el, d_q = (2 |diff| d_diff + d_diff^2) el + diff^2 d_el + 2 E q       <- expf(-lv) times the squared mean difference
        val = (-1 - dd + ed + q) / 2, d_val = (d_dd + d_ed + d_q + 3 E (1 + |dd| + ed + q)) / 2;
        dval = (1 - ed - q) / 2,      d_dval = (d_ed + d_q + 2 E (1 + ed + q)) / 2.
      decoder (t = 0): inv = expf(-lv / 2), d_inv = inv (d_lv / 2 + 4 E);  cen = x0 - mean, d_cen = d_mean + E |cen|;
        a = inv (cen + 1/255), d_a = |a| (d_inv / inv + E) + inv (d_cen + E / 255 + E |cen + 1/255|), b likewise;
        approx_cdf(x): u = k (x + 0.044715 x^3), d_u = 7 E |u|_abs + k (1 + 0.134145 x^2) d_x;  th = tanhf(u), d_th = (1 - th^2) d_u + 4 E |th|;
        cdf = (1 + th) / 2, d_cdf = d_th / 2 + E cdf;  1 - th^2 carries 2 |th| d_th + E;
        pdf = (1 - th^2) k f / 2 with f = 1 + 0.134145 x^2: d_pdf = pdf (8 E + 0.26829 |x| d_x / f) + k f (2 |th| d_th + E) / 2.
        arg = ch | 1 - cl | ch - cl carries d_ch | d_cl + E arg | d_ch + d_cl + E |arg|;  darg = the products ph (-a / 2), pl (-b / 2) with
        their inputs' bounds, E per product and E for the difference.
        val = -logf(arg): d_arg / (arg - d_arg) + 4 E |val|;  dval = -darg / arg: (d_darg + |dval| d_arg) / (arg - d_arg) + E |dval|   <- delta(arg) / arg
        clamped elements (arg < 1e-12): val = -logf(1e-12f) within 4 E |val| + E, dval = 0 EXACTLY.
      grad v half = dval (maxl - minl) / 2 * inv_n * inv_ln2: (|maxl - minl| / 2 / per / ln 2) d_dval + 6 E |ref|.
    sample sums, in the kernel's order (a strided per-thread chain of n_c = ceil(per / 256) additions, 6 shuffle levels, 4 waves):
      mse: (3 + n_c + 10 + 2) E mse (a term (nz - eps)^2 carries 3 E; inv_n and the product 2 E; all terms are non-negative);
      vb:  (sum d_val + (n_c + 10) E sum |val|) / per / ln 2 + 4 E |vb|;   loss == mse + vb bit for bit, and within the sum of the two + E |loss|.
  * training_loss_bwd: one fp32 product and the store: E |ref| + u |ref| (1 + E) + T (u, T: the stored dtype's unit roundoff and subnormal term).
  * diffusion_step.  d_x0 = 2 E (|cr x| + |crm1 eps|) (pred_xstart; the clamp is 1-Lipschitz).
      DDPM: d_frac = E |v + 1| / 2, d_omf = d_frac + E |1 - frac|, d_lv = |maxl| d_frac + |minl| d_omf + 2 E (|frac maxl| + |omf minl|);
        mean carries |c1| d_x0 + 2 E (|c1 x0| + |c2 x|);  s = [t != 0] expf(lv / 2) nz carries |s| (d_lv / 2 + 5 E);  the sum E (|mean| + |s|).
      DDIM: num = cr x - x0 carries E |cr x| + d_x0 + E |num|; eps' = num / crm1 carries d_num / crm1 + E |eps'|     <- the cancellation,
        2^-24 (|cr x| + |x0|) / crm1 and more, largest at small t;  A = 1 - abar_prev, B = 1 - abar carry E each, s1 = sqrtf(A / B) 2.5 E s1;
        C = 1 - abar / abar_prev carries d_C = E abar / abar_prev + E C (C is beta_t: a relative error of E / beta_t), s2 = sqrtf(C) carries
        d_C / (2 s2) + E s2;  sigma = eta s1 s2 carries eta (2.5 E s1 s2 + s1 d_s2) + 2 E sigma;
        D = A - sigma^2 carries E A + 2 sigma d_sigma + E sigma^2 + E D;  sqrtf(D) carries min(d_D / (2 sqrt D), sqrt(d_D)) + E sqrt D;
        t1 = x0 sqrtf(abar_prev): sqrt(abar_prev) d_x0 + 2 E |t1|;  t2 = sqrtf(D) eps': d_sD |eps'| + sqrt(D) d_eps' + E |t2|;
        t3 = [t != 0] sigma nz: |nz| d_sigma + E |t3|;  the two additions 2 E (|t1| + |t2| + |t3|).
  * AdamW (optim.hip:54-65): m and v are double expressions rounded once: E |m|, E |v| (plus 2^-50 of the summands for the double arithmetic).
      denom = sqrtf(v) / sqrtf(bc2) + eps: v's and bc2's own roundings E / 2 each under the root, two sqrtf and the division 2 E each, all
      relative to sq = sqrt(v) / sqrt(bc2): 7 E sq, and the rounded double sum E denom.
      update = step_size m / denom: step_size = lr / bc1 (bc1's rounding and the quotient's: 2 E), m's E, the product E, the division 2 E:
      |update| (6 E + d_denom / denom).  p: E |p - lr wd p| if wd != 0, the update's bound, and the subtraction's E |p|.
      ema, ema_w = (float)(1 - decay) < 0.5: e + ema_w (p - e): ema_w (d_p + E |d|) + 2 E ema_w |d| + E |ema|, d = p - e;
      otherwise p - (p - e)(1 - ema_w): 2 d_p + 3 E |d| + E |ema|.
  Every bound adds F = 2^-100 absolute (the mixer-passes tests' floor) for results in the fp32 denormal range.
MARGIN = 1: the counts above are worst cases and first order, and the second-order terms that matter (d_diff^2, arg - d_arg) are written
out; the fp32 emulation on the CPU needs nothing on top (largest ratios below), so nothing is added.

Largest error-to-bound ratio of the emulation over the prescribed cases (test_emulation_meets_every_bound prints them):
    q_sample          fp32 0.977                            training_loss_bwd fp32 1.000  bf16 0.996  fp16 0.998
    training_loss     fp32 0.952  bf16 0.967  fp16 0.978    diffusion_step    fp32 0.965  bf16 0.958  fp16 0.955
    adamw_ema         fp32 1.000                            grads_nonfinite   exact
(training_loss_bwd in fp32 and AdamW's m and v are ONE rounding against a bound of one rounding; the 16-bit backward is the output's own
half-ulp.)

Seeded defects.  DEFECTS lists the 22 faults of the issue; each, applied to the emulation, exceeds 4 x its bound on at least one
prescribed case (test_seeded_defect_exceeds_four_times_its_bound), with the inputs as first drawn: no seed or case had to be changed.
"""
import math
from types import SimpleNamespace as NS

import numpy as np
import pytest
import torch

from tests.test_mixer_passes_cpu import BF16, CODE, DTYPES, EPS32, F16, F32, FLOOR, NAME, NAN, TINY, UNIT, bits_equal  # noqa: F401

F64 = torch.float64
E = EPS32
MARGIN = 1.0
GRID = 4096 * 256                         # threads of a capped grid-stride launch
INF = float("inf")
LN2 = math.log(2.0)
K_CDF = 0.7978845608028654
NROWS = 14
ROWS = dict(sac="sqrt_alphas_cumprod", s1m="sqrt_one_minus_alphas_cumprod", minl="posterior_log_variance_clipped", maxl="log_betas",
            sr="sqrt_recip_alphas_cumprod", srm1="sqrt_recipm1_alphas_cumprod", c1="posterior_mean_coef1", c2="posterior_mean_coef2",
            ab="alphas_cumprod", abp="alphas_cumprod_prev")
LOSS_ROWS = ("sac", "s1m", "minl", "maxl", "sr", "srm1", "c1", "c2")                # dm_training_loss_args' row_* fields, in order
STEP_ROWS = ("minl", "maxl", "sr", "srm1", "c1", "c2", "ab", "abp")                 # dm_diffusion_step_args' row_* fields, in order
X0_EDGES = [-1.0, -0.9995, -0.999, 0.5, 0.999, 0.9995, 1.0, 1.2]
BAD_T = [-1, None, 2 ** 40]                # None stands for T

RATIOS = {}            # (operator, dtype name) -> largest error / bound the GPU file has seen
_SCHED = {}


def schedule(spec):
    if spec not in _SCHED:
        from diffma_amd.diffusion import create_diffusion

        d = create_diffusion(spec)
        T = d.num_timesteps
        order = torch.randperm(NROWS, generator=torch.Generator().manual_seed(77 + T))[:len(ROWS)].tolist()
        tab = torch.full((NROWS, T), NAN, dtype=F32)
        col, row = {}, {}
        for (k, name), r in zip(ROWS.items(), order):
            col[k] = torch.from_numpy(np.asarray(d._host_table(name), dtype=np.float64)).to(F32)
            tab[r] = col[k]
            row[k] = r
        assert order != sorted(order)
        _SCHED[spec] = NS(spec=spec, T=T, tab=tab, col=col, row=row)
    return _SCHED[spec]


def ratio(got, ref, tol):
    """Largest |got - ref| / tol; inf where an element misses its bound by not being comparable (NaN against a number, a number against
    NaN, a difference against a zero bound)."""
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    tol = torch.as_tensor(tol, dtype=F64).expand(ref.shape) if not torch.is_tensor(tol) else tol.detach().double().reshape(-1).expand(ref.shape)
    if ref.numel() == 0:
        return 0.0
    both_nan = got.isnan() & ref.isnan()
    err = (got - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / (tol * MARGIN))
    r = torch.where(both_nan, torch.zeros_like(r), r)
    r = torch.where(r.isnan(), torch.full_like(r, INF), r)
    return float(r.max())


def judge(op, dt, res, book=None, strict=True):
    """res: name -> ratio.  Asserts every ratio <= 1 (strict) and books the largest."""
    worst = max(res.values()) if res else 0.0
    if strict:
        bad = {k: v for k, v in res.items() if not v <= 1.0}
        assert not bad, f"{op} {NAME[dt]}: out of bound (error / bound): {bad}"
        book = RATIOS if book is None else book
        book[(op, NAME[dt])] = max(book.get((op, NAME[dt]), 0.0), worst)
    return worst


def _flat_index(B, per, stride, defect):
    """(b, r) of the elements e = 0 .. B * stride - 1 of a grid-stride loop; defect 1: second-trip elements keep the first trip's b."""
    e = torch.arange(B * stride)
    b = e // stride
    if defect == "stale_b" and e.numel() > GRID:
        b = torch.cat([b[:GRID], b[:e.numel() - GRID]])
    return b, e - b * stride


def _tcol(s, k, t, D):
    return s.col[k][t.clamp(0, s.T - 1)].to(D)


def _mixed_t(T, B, g):
    t = torch.randint(1, T - 1, (B,), generator=g)
    t[0] = 0
    t[-1] = T - 1
    if B > 2:
        t[B // 2] = 1
    return t


# =====================================================================================================================================
# dm_q_sample
# =====================================================================================================================================
def qs_case(spec, B, C, hw, t=None, seed=0):
    s = schedule(spec)
    g = torch.Generator().manual_seed(seed)
    per = C * hw
    t = _mixed_t(s.T, B, g) if t is None else torch.as_tensor(t, dtype=torch.int64)
    return NS(s=s, B=B, C=C, hw=hw, per=per, t=t, x0=torch.randn(B, per, generator=g), nz=torch.randn(B, per, generator=g))


def qs_math(c, D, defect=None):
    b, _ = _flat_index(c.B, c.per, c.per, defect)
    t = c.t[b]
    a, s1 = _tcol(c.s, "sac", t, D), _tcol(c.s, "s1m", t, D)
    if defect == "swap_recip":
        a, s1 = s1, a
    p1, p2 = a * c.x0.reshape(-1).to(D), s1 * c.nz.reshape(-1).to(D)
    out = p1 + p2
    out[(t < 0) | (t >= c.s.T)] = NAN
    return NS(out=out.view(c.B, c.per), p1=p1, p2=p2)


def qs_emul(c, defect=None):
    return qs_math(c, F32, defect).out


def qs_eval(c, out, book=None, strict=True):
    R = qs_math(c, F64)
    tol = (2 * E * (R.p1.abs() + R.p2.abs()) + FLOOR).view(c.B, c.per)
    return judge("q_sample", F32, {"x_t": ratio(out, R.out, tol)}, book, strict)


# =====================================================================================================================================
# dm_training_loss
# =====================================================================================================================================
def tl_case(dt, spec, B, C, hw, t=None, seed=0, pops=None):
    """model_out (eps | v) in dt, x0 / x_t / noise fp32.  Samples at t = 0 are constructed so that no element sits near
    the clamp of the decoder term, where fp32 and fp64 could disagree on the side (coef1 = 1 and coef2 = 0 there): x0 cycles through X0_EDGES, eps = (sr x_t - x0 + cen) / srm1 puts the discretised-decoder window at `cen`;
    live elements |cen| <= 2 / inv_hi (arg >= 1e-4 in fp64), dead ones 14 / inv_lo <= |cen| <= 28 / inv_lo on the side where both cdfs
    saturate (|a|, |b| >= 10), inv = exp(-logvar / 2) between inv_lo and inv_hi since v is kept in [-1, 1] there.  pops[b] in
    {"mixed", "live", "dead"} (default mixed: alternating groups of 8)."""
    s = schedule(spec)
    g = torch.Generator().manual_seed(seed)
    per = C * hw
    t = _mixed_t(s.T, B, g) if t is None else torch.as_tensor(t, dtype=torch.int64)
    x0 = torch.randn(B, per, generator=g).clamp(-1.2, 1.2)
    nz = torch.randn(B, per, generator=g)
    xt = qs_emul(NS(s=s, B=B, per=per, t=t.clamp(0, s.T - 1), x0=x0, nz=nz))
    eps = torch.randn(B, per, generator=g, dtype=F64)
    v = torch.randn(B, per, generator=g, dtype=F64).clamp(-1.5, 1.5)
    dead = torch.zeros(B, per, dtype=torch.bool)
    r = torch.arange(per)
    for b in range(B):
        if int(t[b]) != 0:
            continue
        pop = (pops[b] if pops else "mixed")
        x0[b] = torch.tensor(X0_EDGES)[r % 8]
        xt[b] = qs_emul(NS(s=s, B=1, per=per, t=t[b:b + 1], x0=x0[b:b + 1], nz=nz[b:b + 1]))[0]
        v[b] = v[b].clamp(-1.0, 1.0)
        dead[b] = {"mixed": (r // 8) % 2 == 1, "live": torch.zeros(per, dtype=torch.bool), "dead": torch.ones(per, dtype=torch.bool)}[pop]
        maxl, minl = float(s.col["maxl"][0]), float(s.col["minl"][0])
        inv_lo, inv_hi = math.exp(-0.5 * max(maxl, minl)), math.exp(-0.5 * min(maxl, minl))
        u = torch.rand(per, generator=g, dtype=F64)
        sgn = torch.where(torch.rand(per, generator=g) < 0.5, -1.0, 1.0).double()
        sgn = torch.where(x0[b] < -0.999, -torch.ones_like(sgn), torch.where(x0[b] > 0.999, torch.ones_like(sgn), sgn))
        cen = torch.where(dead[b], sgn * (14 + 14 * u) / inv_lo, (2 * u - 1) * 2.0 / inv_hi)
        sr, srm1 = float(s.col["sr"][0]), float(s.col["srm1"][0])
        eps[b] = (sr * xt[b].double() - x0[b].double() + cen) / srm1
    mo = torch.cat([eps, v], dim=1).to(dt)
    return NS(dt=dt, s=s, B=B, C=C, hw=hw, per=per, t=t, x0=x0, xt=xt, nz=nz, mo=mo, dead=dead, is0=(t == 0))


def _cdf(x, D):
    th = torch.tanh(K_CDF * (x + 0.044715 * x * x * x))
    return 0.5 * (1.0 + th), 0.5 * (1.0 - th * th) * K_CDF * (1.0 + (3.0 * 0.044715) * x * x), th


def _sample_sum(x, D):
    """Sum over dim 1 in training_loss_kernel's order (fp32), or exactly (fp64)."""
    if D == F64:
        return x.sum(1)
    B, per = x.shape
    nc = -(-per // 256)
    pad = torch.zeros(B, nc * 256, dtype=D)
    pad[:, :per] = x
    pad = pad.view(B, nc, 256)
    acc = torch.zeros(B, 256, dtype=D)
    for i in range(nc):
        acc = acc + pad[:, i]
    w = acc.view(B, 4, 64).clone()
    for off in (32, 16, 8, 4, 2, 1):
        w[..., :off] = w[..., :off] + w[..., off:2 * off]
    tot = torch.zeros(B, dtype=D)
    for k in range(4):
        tot = tot + w[:, k, 0]
    return tot


def tl_math(c, D, defect=None):
    s, per, dt = c.s, c.per, c.dt
    t = c.t
    bad = (t < 0) | (t >= s.T)
    col = {k: _tcol(s, k, t, D)[:, None] for k in LOSS_ROWS}
    sr, srm1, minl, maxl, c1, c2 = (col[k] for k in ("sr", "srm1", "minl", "maxl", "c1", "c2"))
    if defect == "swap_coef":
        c1, c2 = c2, c1
    if defect == "swap_recip":
        sr, srm1 = srm1, sr
    if defect == "swap_log":
        minl, maxl = maxl, minl
    one = torch.tensor(1.0, dtype=D)
    inv_n = one / torch.tensor(float(per), dtype=D)
    inv_ln2 = torch.tensor(1.4426950408889634, dtype=D)
    eps, v = c.mo[:, :per].to(D), c.mo[:, per:].to(D)
    x0, xt, nz = c.x0.to(D), c.xt.to(D), c.nz.to(D)
    rnd = (lambda x: x) if defect == "frac_unrounded" else (lambda x: x.float().to(dt).to(D))
    d = nz - eps
    g_eps = -2.0 * d * inv_n
    frac = rnd(v + 1.0) * 0.5
    omf = rnd(1.0 - frac)
    lv = frac * maxl + omf * minl
    px0 = sr * xt - srm1 * eps
    mean, tmean = c1 * px0 + c2 * xt, c1 * x0 + c2 * xt
    # KL
    dd = minl - lv
    ed, el = torch.exp(dd), torch.exp(-lv)
    diff = tmean - mean
    q = diff * diff * el
    val_kl, dval_kl = 0.5 * (-1.0 - dd + ed + q), 0.5 * (1.0 - ed - q)
    # discretised decoder
    inv, cen = torch.exp(-0.5 * lv), x0 - mean
    c255 = one / 255.0
    a, bb = inv * (cen + c255), inv * (cen - c255)
    ch, ph, tha = _cdf(a, D)
    cl, pl, thb = _cdf(bb, D)
    thr = torch.tensor(0.999, dtype=F32).to(D)
    left = (x0 < thr) if defect == "left_branch_wide" else (x0 < -thr)
    right = (x0 > thr) & ~left
    da_l, da_r = ph * (-0.5 * a), -pl * (-0.5 * bb)
    arg = torch.where(left, ch, torch.where(right, 1.0 - cl, ch - cl))
    darg = torch.where(left, da_l, torch.where(right, da_r, ph * (-0.5 * a) - pl * (-0.5 * bb)))
    floor = torch.tensor(1e-12, dtype=F32).to(D)
    live = arg >= floor
    val_dec = -torch.log(torch.where(live, arg, floor))
    dval_dec = -darg / arg if defect == "clamp_grad_live" else torch.where(live, -darg / torch.where(live, arg, one), torch.zeros_like(arg))
    is0 = (t == 0)[:, None]
    val, dval = torch.where(is0, val_dec, val_kl), torch.where(is0, dval_dec, dval_kl)
    g_v = dval * inv_n * inv_ln2 if defect == "no_range_factor" else dval * 0.5 * (maxl - minl) * inv_n * inv_ln2
    mse = _sample_sum(d * d, D) * inv_n
    vb = _sample_sum(val, D) * (inv_n if defect == "no_ln2" else inv_n * inv_ln2)
    loss = mse + vb
    grad = torch.cat([g_eps, g_v], dim=1)
    grad[bad] = NAN
    for x in (mse, vb, loss):
        x[bad] = NAN
    return NS(**{k: w for k, w in locals().items() if torch.is_tensor(w)})


def tl_emul(c, defect=None):
    R = tl_math(c, F32, defect)
    return R.mse, R.vb, R.loss, R.grad


def tl_bounds(c, R):
    A = torch.abs
    per = c.per
    d_lv = 2 * E * (A(R.frac * R.maxl) + A(R.omf * R.minl))
    d_px0 = 2 * E * (A(R.sr * R.xt) + A(R.srm1 * R.eps))
    d_mean = A(R.c1) * d_px0 + 2 * E * (A(R.c1 * R.px0) + A(R.c2 * R.xt))
    d_tmean = 2 * E * (A(R.c1 * R.x0) + A(R.c2 * R.xt))
    # KL
    d_diff = d_mean + d_tmean + E * A(R.diff)
    d_dd = d_lv + E * A(R.dd)
    d_ed, d_el = R.ed * (d_dd + 4 * E), R.el * (d_lv + 4 * E)
    d_q = (2 * A(R.diff) * d_diff + d_diff ** 2) * R.el + R.diff ** 2 * d_el + 2 * E * R.q
    mag = 1 + A(R.dd) + R.ed + R.q
    d_val_kl = 0.5 * (d_dd + d_ed + d_q + 3 * E * mag)
    d_dval_kl = 0.5 * (d_ed + d_q + 2 * E * (1 + R.ed + R.q))
    # decoder
    d_inv = R.inv * (0.5 * d_lv + 4 * E)
    d_cen = d_mean + E * A(R.cen)

    def d_edge(x, off):
        return A(x) * (d_inv / R.inv + E) + R.inv * (d_cen + E / 255 + E * A(R.cen + off))

    def d_cdf(x, d_x, th, cdf, pdf):
        f = 1 + 3 * 0.044715 * x * x
        d_u = 7 * E * K_CDF * (A(x) + 0.044715 * A(x) ** 3) + K_CDF * f * d_x
        d_th = (1 - th * th) * d_u + 4 * E * A(th)
        d_omt = 2 * A(th) * d_th + E
        return 0.5 * d_th + E * cdf, pdf * (8 * E + 2 * 3 * 0.044715 * A(x) * d_x / f) + 0.5 * K_CDF * f * d_omt

    d_a, d_b = d_edge(R.a, 1 / 255), d_edge(R.bb, -1 / 255)
    d_ch, d_ph = d_cdf(R.a, d_a, R.tha, R.ch, R.ph)
    d_cl, d_pl = d_cdf(R.bb, d_b, R.thb, R.cl, R.pl)
    d_l = 0.5 * (A(R.a) * d_ph + R.ph * d_a)
    d_r = 0.5 * (A(R.bb) * d_pl + R.pl * d_b)
    d_arg = torch.where(R.left, d_ch, torch.where(R.right, d_cl + E * A(R.arg), d_ch + d_cl + E * A(R.arg)))
    d_darg = torch.where(R.left, d_l + E * A(R.da_l), torch.where(R.right, d_r + E * A(R.da_r),
                                                                   d_l + d_r + E * (A(R.da_l) + A(R.da_r)) + E * A(R.darg)))
    arg_lo = (R.arg - d_arg).clamp_min(1e-300)
    d_val_dec = torch.where(R.live, d_arg / arg_lo + 4 * E * A(R.val_dec), 4 * E * A(R.val_dec) + E)
    d_dval_dec = torch.where(R.live, (d_darg + A(R.dval_dec) * d_arg) / arg_lo + E * A(R.dval_dec), torch.zeros_like(R.arg))
    d_val = torch.where(R.is0, d_val_dec, d_val_kl)
    d_dval = torch.where(R.is0, d_dval_dec, d_dval_kl)
    n_sum = -(-per // 256) + 10
    K = 0.5 * A(R.maxl - R.minl) / per / LN2
    g_v = K * d_dval + 6 * E * A(R.g_v)
    g_v = torch.where(R.is0 & ~R.live, torch.zeros_like(g_v), g_v + FLOOR)                 # clamped: exactly 0
    return NS(g_eps=3 * E * A(R.g_eps) + FLOOR, g_v=g_v, mse=(3 + n_sum + 2) * E * R.mse + FLOOR,
              vb=(d_val.sum(1) + n_sum * E * A(R.val).sum(1)) / per / LN2 + 4 * E * A(R.vb) + FLOOR)


def tl_eval(c, mse, vb, loss, grad, book=None, strict=True, op="training_loss"):
    R = tl_math(c, F64)
    T = tl_bounds(c, R)
    per = c.per
    nan = torch.full_like(T.mse, NAN)
    bad = R.bad
    res = {"mse": ratio(mse, R.mse, torch.where(bad, nan, T.mse)), "vb": ratio(vb, R.vb, torch.where(bad, nan, T.vb)),
           "loss": ratio(loss, R.loss, torch.where(bad, nan, T.mse + T.vb + E * R.loss.abs())),
           "grad_eps": ratio(grad[:, :per], R.grad[:, :per], T.g_eps), "grad_v": ratio(grad[:, per:], R.grad[:, per:], T.g_v)}
    if strict:
        assert bits_equal(loss.float(), (mse.float() + vb.float())), "loss != mse + vb bit for bit"
    return judge(op, c.dt, res, book, strict)


def tl_sides(c):
    """The condition of the `t = 0 decoder inputs` paragraph: every t = 0 element on its intended side, in fp64 and in the emulation."""
    R64, R32 = tl_math(c, F64), tl_math(c, F32)
    m = c.is0[:, None].expand_as(c.dead)
    live, dead = m & ~c.dead, m & c.dead
    assert bool((R64.arg[live] >= 1e-4).all()) and bool(R32.live[live].all())
    assert bool((R64.a[dead].abs() >= 10).all()) and bool((R64.bb[dead].abs() >= 10).all())
    assert bool((R64.arg[dead] < 1e-12).all()) and bool((R32.arg[dead] == 0).all())
    want = -math.log(float(torch.tensor(1e-12, dtype=F32)))
    assert bool(((R32.val_dec[dead].double() - want).abs() <= 2.0 ** -19).all())          # an ulp of 27.6
    assert bool((R32.dval_dec[dead] == 0).all()) and bool((R32.g_v[dead] == 0).all())
    mid = ~R64.left & ~R64.right
    br = {k: (int((w & R64.left).sum()), int((w & R64.right).sum()), int((w & mid).sum())) for k, w in (("live", live), ("dead", dead))}
    return int(live.sum()), int(dead.sum()), br


# =====================================================================================================================================
# dm_training_loss_bwd
# =====================================================================================================================================
def lb_case(dt, B, C, hw, seed=0):
    g = torch.Generator().manual_seed(seed)
    per = C * hw
    grad = torch.randn(B, 2 * per, generator=g) * 10.0 ** torch.randint(-6, 1, (B, 2 * per), generator=g).float()
    grad[:, ::97] = 0.0
    g_eps = torch.linspace(0.5, 1.5, B)
    g_v = torch.linspace(-1.25, 0.75, B)
    g_eps[B // 2], g_v[0] = 0.0, -0.375
    if B > 2:
        g_eps[-1], g_v[1] = -2.0, 0.0
    return NS(dt=dt, B=B, C=C, hw=hw, per=per, grad=grad, g_eps=g_eps, g_v=g_v)


def lb_math(c, D, defect=None):
    b, r = _flat_index(c.B, c.per, 2 * c.per, defect)
    is_v = r >= c.per
    ge, gv = (c.g_v, c.g_eps) if defect == "swap_g" else (c.g_eps, c.g_v)
    g = torch.where(is_v, gv[b], ge[b]).to(D)
    return (g * c.grad.reshape(-1).to(D)).view(c.B, 2 * c.per)


def lb_emul(c, defect=None):
    return lb_math(c, F32, defect).to(c.dt)


def lb_eval(c, out, book=None, strict=True):
    ref = lb_math(c, F64)
    tol = E * ref.abs() + UNIT[c.dt] * ref.abs() * (1 + E) + TINY[c.dt] + FLOOR
    return judge("training_loss_bwd", c.dt, {"grad_out": ratio(out, ref, tol)}, book, strict)


# =====================================================================================================================================
# dm_diffusion_step
# =====================================================================================================================================
def ds_case(dt, spec, B, C, hw, mode, eta=0.0, clip=0, t=None, seed=0, noise=True):
    """x = 1.5 N(0, 1): x0 = cr x - crm1 eps leaves [-1, 1] on both sides at every t (crm1 grows to 150 at the end of the schedule)."""
    s = schedule(spec)
    g = torch.Generator().manual_seed(seed)
    per = C * hw
    t = _mixed_t(s.T, B, g) if t is None else torch.as_tensor(t, dtype=torch.int64)
    x = 1.5 * torch.randn(B, per, generator=g)
    nz = torch.randn(B, per, generator=g)
    mo = torch.cat([torch.randn(B, per, generator=g), torch.randn(B, per, generator=g).clamp(-1.5, 1.5)], dim=1).to(dt)
    return NS(dt=dt, s=s, B=B, C=C, hw=hw, per=per, mode=mode, eta=float(eta), clip=int(clip), t=t, x=x, nz=nz if noise else None, mo=mo)


def ds_math(c, D, defect=None):
    s, per = c.s, c.per
    b, r = _flat_index(c.B, per, per, defect)
    t = c.t[b]
    bad = (t < 0) | (t >= s.T)
    col = {k: _tcol(s, k, t, D) for k in STEP_ROWS}
    cr, crm1, minl, maxl, c1, c2, ab, abp = (col[k] for k in ("sr", "srm1", "minl", "maxl", "c1", "c2", "ab", "abp"))
    if defect == "swap_coef":
        c1, c2 = c2, c1
    if defect == "swap_recip":
        cr, crm1 = crm1, cr
    if defect == "swap_log":
        minl, maxl = maxl, minl
    if defect == "abp_at_t":
        abp = ab
    mo = c.mo.reshape(-1)
    i_eps = (b * 2 * per + r).clamp(max=mo.numel() - per - 1)
    eps, v = mo[i_eps].to(D), mo[i_eps + per].to(D)
    x = c.x.reshape(-1).to(D)
    nz = c.nz.reshape(-1).to(D) if c.nz is not None else torch.zeros_like(x)
    eta = 0.0 if defect == "no_eta" else torch.tensor(c.eta, dtype=F32).to(D)
    vp1 = v + 1.0
    frac = vp1 * 0.5
    omf = 1.0 - frac
    lv = frac * maxl + omf * minl
    p1, p2 = cr * x, crm1 * eps
    x0 = p1 - p2
    if c.clip and defect != "no_clip":
        x0 = x0.clamp(-1.0, 1.0)
    mask = torch.ones_like(x) if defect == "no_mask" else (t != 0).to(D)
    if c.mode == 0:
        mean = c1 * x0 + c2 * x
        sd = torch.exp(0.5 * lv)
        term = mask * sd * nz
        sample = mean + term
    else:
        num = p1 - x0
        eps2 = num / crm1
        A_, B_ = 1.0 - abp, 1.0 - ab
        s1 = torch.sqrt(A_ / B_)
        Rr = ab / abp
        Cc = 1.0 - Rr
        s2 = torch.sqrt(Cc)
        sigma = eta * s1 * s2
        D_ = A_ - sigma * sigma
        sD = torch.sqrt(D_)
        sab = torch.sqrt(abp)
        t1, t2, t3 = x0 * sab, sD * eps2, mask * sigma * nz
        sample = t1 + t2 + t3
    sample, x0 = sample.clone(), x0.clone()
    sample[bad] = NAN
    x0[bad] = NAN
    return NS(**{k: w for k, w in locals().items() if torch.is_tensor(w)})


def ds_emul(c, defect=None):
    R = ds_math(c, F32, defect)
    return R.sample.view(c.B, c.per), R.x0.view(c.B, c.per)


def ds_bounds(c, R):
    A = torch.abs
    d_x0 = 2 * E * (A(R.p1) + A(R.p2))
    if c.mode == 0:
        d_frac = 0.5 * E * A(R.vp1)
        d_omf = d_frac + E * A(R.omf)
        d_lv = A(R.maxl) * d_frac + A(R.minl) * d_omf + 2 * E * (A(R.frac * R.maxl) + A(R.omf * R.minl))
        d_mean = A(R.c1) * d_x0 + 2 * E * (A(R.c1 * R.x0) + A(R.c2 * R.x))
        d_term = A(R.term) * (0.5 * d_lv + 5 * E)
        tol = d_mean + d_term + E * (A(R.mean) + A(R.term))
    else:
        d_num = E * A(R.p1) + d_x0 + E * A(R.num)
        d_eps2 = d_num / R.crm1 + E * A(R.eps2)
        d_C = E * R.Rr + E * R.Cc
        d_s2 = 0.5 * d_C / R.s2 + E * R.s2
        d_sigma = R.eta * (2.5 * E * R.s1 * R.s2 + R.s1 * d_s2) + 2 * E * R.sigma
        d_D = E * R.A_ + 2 * R.sigma * d_sigma + E * R.sigma ** 2 + E * A(R.D_)
        d_sD = torch.minimum(0.5 * d_D / R.sD.clamp_min(1e-300), torch.sqrt(d_D)) + E * R.sD
        d_t1 = R.sab * d_x0 + 2 * E * A(R.t1)
        d_t2 = d_sD * A(R.eps2) + R.sD * d_eps2 + E * A(R.t2)
        d_t3 = A(R.nz) * R.mask * d_sigma + E * A(R.t3)
        tol = d_t1 + d_t2 + d_t3 + 2 * E * (A(R.t1) + A(R.t2) + A(R.t3))
    return tol + FLOOR, d_x0 + FLOOR


def ds_eval(c, sample, x0, book=None, strict=True):
    R = ds_math(c, F64)
    t_s, t_x = ds_bounds(c, R)
    res = {"sample": ratio(sample, R.sample, t_s)}
    if x0 is not None:
        res["pred_xstart"] = ratio(x0, R.x0, t_x)
    if strict:
        ok = ~R.bad
        assert bool(sample.reshape(-1)[ok].isfinite().all()), "diffusion_step: a non-finite sample at a valid timestep"
    return judge("diffusion_step", c.dt, res, book, strict)


# =====================================================================================================================================
# dm_adamw_ema_step
# =====================================================================================================================================
AW_CHUNK = 4096
AW_COUNTERS = [0.0, 9.0, 999.0, 99999.0]


def aw_sizes(chunk=AW_CHUNK):
    return [1, 3, 4, 5, 1023, chunk, chunk + 1, 2 * chunk + 3]


def aw_case(seed=0, chunk=AW_CHUNK, no_ema=(2,), no_step=(4,)):
    """The table: one tensor per size of aw_sizes; gradient magnitudes graded from 1e-20 to 1e4, m and v carried over from gradients of
    the same magnitude; the first two elements of every tensor of 3 or more have g = m = v = 0 (the update must be exactly 0);
    rows `no_ema` have ema == NULL, rows `no_step` have step == NULL (t = 1)."""
    g = torch.Generator().manual_seed(seed)
    ts = []
    for i, n in enumerate(aw_sizes(chunk)):
        gs = 10.0 ** (torch.rand(n, generator=g, dtype=F64) * 24 - 20)
        gr = (torch.randn(n, generator=g, dtype=F64) * gs).float()
        m = (0.5 * torch.randn(n, generator=g, dtype=F64) * gs).float()
        v = ((0.7 * gs) ** 2 * torch.rand(n, generator=g, dtype=F64)).float()
        p = torch.randn(n, generator=g)
        ema = None if i in no_ema else (p + 0.1 * torch.randn(n, generator=g))
        if n >= 3:
            gr[:2], m[:2], v[:2] = 0.0, 0.0, 0.0
        step = None if i in no_step else torch.tensor(AW_COUNTERS[i % 4])
        ts.append(NS(n=n, p=p, m=m, v=v, g=gr, ema=ema, step=step))
    bt, bc = [], []
    for i, t in enumerate(ts):
        nb = -(-t.n // chunk)
        bt += [i] * nb
        bc += list(range(nb))
    perm = torch.randperm(len(bt), generator=g).tolist()
    assert perm != sorted(perm)
    return NS(ts=ts, chunk=chunk, bt=[bt[i] for i in perm], bc=[bc[i] for i in perm])


def aw_hp(lr=1e-4, wd=0.0, decay=0.9999, found=None, ema_on_skip=1, b1=0.9, b2=0.999, eps=1e-8):
    return NS(lr=lr, wd=wd, decay=decay, found=found, ema_on_skip=ema_on_skip, b1=b1, b2=b2, eps=eps)


def aw_emul(c, hp, defect=None):
    """The new (p, m, v, ema, step) of every tensor, as adamw_ema_kernel computes them (optim.hip:54-65, 92-96)."""
    out = []
    skip = hp.found is not None and hp.found != 0.0
    ema_on = (not skip) or hp.ema_on_skip != 0
    f32 = lambda x: torch.tensor(x, dtype=F64).float()
    for i, T in enumerate(c.ts):
        p, m, v, ema, step = T.p.clone(), T.m.clone(), T.v.clone(), None if T.ema is None else T.ema.clone(), None if T.step is None else T.step.clone()
        n_upd = T.n - T.n % 4 if defect == "skip_tail" else T.n
        sl = slice(0, n_upd)
        w = p[sl].clone()
        if not skip:
            if step is not None:
                step += 1.0
            src = c.ts[0].step + 1.0 if (defect == "one_step_for_all" and c.ts[0].step is not None) else step
            t = float(src) if src is not None else 1.0
            if defect == "bias_before_increment":
                t -= 1.0
            bc1, bc2 = f32(1.0 - hp.b1 ** t), f32(1.0 - hp.b2 ** t)
            bc2_sqrt = torch.sqrt(bc2)
            step_size = (hp.lr / bc1.double()).float()
            gd = T.g[sl].double()
            if hp.wd != 0.0 and defect != "wd_after":
                w = (w.double() - hp.lr * hp.wd * w.double()).float()
            m[sl] = (hp.b1 * m[sl].double() + (1.0 - hp.b1) * gd).float()
            v[sl] = (hp.b2 * v[sl].double() + (1.0 - hp.b2) * gd * gd).float()
            sq = torch.sqrt(v[sl]) if defect == "no_bc2" else torch.sqrt(v[sl]) / bc2_sqrt
            denom = (sq.double() + hp.eps).float()
            w = w - step_size * m[sl] / denom
            if hp.wd != 0.0 and defect == "wd_after":
                w = (w.double() - hp.lr * hp.wd * w.double()).float()
        if ema is not None and ema_on:
            ew = f32(1.0 - hp.decay)
            src = p[sl] if defect == "ema_old_weight" else w
            e = ema[sl]
            ema[sl] = e + ew * (src - e) if float(ew) < 0.5 else src - (src - e) * (1.0 - ew)
        if not skip:
            p[sl] = w
        out.append(NS(p=p, m=m, v=v, ema=ema, step=step))
    return out


def aw_eval(c, hp, outs, book=None, strict=True):
    """outs[i]: NS(p, m, v, ema, step) after the call."""
    skip = hp.found is not None and hp.found != 0.0
    ema_on = (not skip) or hp.ema_on_skip != 0
    res = {}
    A = torch.abs

    def put(k, r):
        res[k] = max(res.get(k, 0.0), r)

    def same(k, got, want):
        put(k, 0.0 if bits_equal(got, want) else INF)

    for T, o in zip(c.ts, outs):
        p0 = T.p.double()
        if skip:
            same("p", o.p, T.p), same("m", o.m, T.m), same("v", o.v, T.v)
            if T.step is not None:
                same("step", o.step, T.step)
            p_ref, d_p = p0, torch.zeros_like(p0)
        else:
            t = float(T.step) + 1.0 if T.step is not None else 1.0
            if T.step is not None:
                same("step", o.step, torch.tensor(t, dtype=F32))
            g, m0, v0 = T.g.double(), T.m.double(), T.v.double()
            m = hp.b1 * m0 + (1.0 - hp.b1) * g
            v = hp.b2 * v0 + (1.0 - hp.b2) * g * g
            bc1, bc2 = 1.0 - hp.b1 ** t, 1.0 - hp.b2 ** t
            sq = torch.sqrt(v) / math.sqrt(bc2)
            den = sq + hp.eps
            ss = hp.lr / bc1
            upd = ss * m / den
            pw = p0 - hp.lr * hp.wd * p0
            p_ref = pw - upd
            d_den = 7 * E * sq + E * den + 2.0 ** -50
            d_upd = A(upd) * (6 * E + d_den / den) + ss * FLOOR / den
            d_p = (E * A(pw) if hp.wd != 0.0 else 0.0) + d_upd + E * A(p_ref) + FLOOR
            dbl = 2.0 ** -50                                # the double expressions' own roundings, whatever their order or contraction
            put("m", ratio(o.m, m, E * A(m) + dbl * (A(hp.b1 * m0) + A((1.0 - hp.b1) * g)) + FLOOR))
            put("v", ratio(o.v, v, (E + dbl) * A(v) + FLOOR))
            put("p", ratio(o.p, p_ref, d_p))
            if strict:
                z = (T.g == 0) & (T.v == 0) & (T.m == 0)
                if hp.wd == 0.0 and bool(z.any()):
                    assert bits_equal(o.p[z], T.p[z]), "g = m = v = 0: the update must be exactly 0"
        if T.ema is None:
            assert o.ema is None
            continue
        if not ema_on:
            same("ema", o.ema, T.ema)
            continue
        e0 = T.ema.double()
        ew64 = 1.0 - hp.decay
        ew32 = float(torch.tensor(ew64, dtype=F64).float())
        e_ref = e0 + ew64 * (p_ref - e0)
        d = A(p_ref - e0)
        tol = (ew32 * (d_p + E * d) + 2 * E * ew32 * d if ew32 < 0.5 else 2 * d_p + 3 * E * d) + E * A(e_ref) + FLOOR
        put("ema", ratio(o.ema, e_ref, tol))
        if strict and hp.decay == 0.0:
            assert bits_equal(o.ema, o.p), "ema_decay 0: ema == p bit for bit"
        if strict and hp.decay == 1.0:
            assert bits_equal(o.ema, T.ema), "ema_decay 1: ema unchanged bit for bit"
    return judge("adamw_ema", F32, res, book, strict)


# =====================================================================================================================================
# dm_grads_nonfinite
# =====================================================================================================================================
def nf_positions(chunk=AW_CHUNK):
    """(tensor index of aw_sizes, element) of every planting position of the issue's list."""
    sz = aw_sizes(chunk)
    big = len(sz) - 1                                                  # 2 chunk + 3: last tensor of the table, tail of 3
    pos = [(big, 0)] + [(big, 40 + j) for j in range(4)] + [(big, chunk - 1), (big, chunk)] + [(big, 2 * chunk + j) for j in range(3)]
    pos += [(1, j) for j in range(3)] + [(3, 4), (6, chunk), (0, 0)]      # tails of n = 3, 5, chunk + 1; the single element
    return pos


def nf_case(plant=None, value=None, chunk=AW_CHUNK, seed=0):
    g = torch.Generator().manual_seed(seed)
    gs = [torch.randn(n, generator=g) for n in aw_sizes(chunk)]
    edge = torch.tensor([3.4e38, -3.4e38, 1e-40, -1e-45, -0.0, 0.0])
    for x in gs:
        k = min(x.numel(), edge.numel())
        x[-k:] = edge[:k]
    if plant is not None:
        gs[plant[0]][plant[1]] = value
    return gs


def nf_emul(gs, aligned=True, defect=None):
    """grads_nonfinite_kernel: x - x summed over a 16-byte vector where g is aligned and four elements are left, element-wise otherwise."""
    bad = False
    for x in gs:
        n = x.numel()
        if defect == "blind_neg_inf":
            bad = bad or bool(((x != x) | (x > 3.4028234e38)).any())
            continue
        nv = (n // 4) * 4 if aligned else 0
        if nv:
            q = x[:nv].view(-1, 4)
            z = (q[:, 0] - q[:, 0]) + (q[:, 1] - q[:, 1]) + (q[:, 2] - q[:, 2]) + (q[:, 3] - q[:, 3])
            bad = bad or bool((~(z == 0)).any())
        tail = x[nv:n - n % 4] if defect == "blind_tail" else x[nv:]
        bad = bad or bool((~((tail - tail) == 0)).any())
    return 1.0 if bad else 0.0


def nf_eval(gs, got, book=None, strict=True):
    want = 0.0 if all(bool(x.isfinite().all()) for x in gs) else 1.0
    return judge("grads_nonfinite", F32, {"flag": 0.0 if float(got) == want else INF}, book, strict)


# =====================================================================================================================================
# The prescribed cases, shared with the GPU file
# =====================================================================================================================================
SPECS = ["", "250"]
TL_PERS = [(1, 1), (1, 63), (1, 255), (4, 64), (1, 257), (4, 784)]         # (C, hw): per 1, 63, 255, 256, 257, 3136


def qs_cases():
    out = []
    for spec in SPECS:
        T = schedule(spec).T
        out += [qs_case(spec, 5, 3, 7, seed=1), qs_case(spec, T, 1, 8, t=torch.arange(T), seed=2)]
    out.append(qs_case("", 3, 1, 350003, t=[0, 517, 999], seed=3))
    return out


def tl_cases(dt, big=True):
    out = []
    for spec in SPECS:
        T = schedule(spec).T
        for C, hw in TL_PERS:
            out += [tl_case(dt, spec, 1, C, hw, t=[0 if hw % 2 else T // 3], seed=10 + hw), tl_case(dt, spec, 7, C, hw, seed=20 + hw)]
        out.append(tl_case(dt, spec, T, 1, 8, t=torch.arange(T), seed=30))
        out.append(tl_case(dt, spec, 3, 4, 784, t=[0, 0, 0], seed=31, pops=["live", "dead", "mixed"]))
        out += [tl_case(dt, spec, 1, 1, 1, t=[0], seed=33 + i, pops=["dead"]) for i in range(3)]       # vb IS one clamped element's value
    if big:
        out.append(tl_big(dt))
    return out


def tl_big(dt):
    """per = 175 003: a per-thread chain of 684 additions in the sample sums."""
    return tl_case(dt, "", 2, 1, 175003, t=[0, 400], seed=32)


def lb_cases(dt):
    return [lb_case(dt, 5, 3, 7, seed=40), lb_case(dt, 3, 1, 175003, seed=41)]


def ds_modes():
    return [(0, 0.0), (1, 0.0), (1, 0.5), (1, 1.0)]


def ds_cases(dt, big=True):
    out = []
    for spec in SPECS:
        T = schedule(spec).T
        for mode, eta in ds_modes():
            for clip in (0, 1):
                out.append(ds_case(dt, spec, T, 1, 8, mode, eta, clip, t=torch.arange(T), seed=50 + mode))
                out.append(ds_case(dt, spec, 5, 3, 7, mode, eta, clip, seed=51 + clip))
    if big:
        out += ds_big(dt)
    return out


def ds_big(dt):
    """1 050 009 elements: the last 1433 take the second grid-stride trip; sample boundaries fall inside a workgroup."""
    return [ds_case(dt, "", 3, 1, 350003, mode, eta, 1, t=[0, 3, 999], seed=52) for mode, eta in ((0, 0.0), (1, 0.5))]


def aw_hps():
    out = [aw_hp(lr=lr, wd=wd, decay=dec) for lr in (1e-4, 1e-2) for wd in (0.0, 0.01) for dec in (0.9, 0.9999)]
    out += [aw_hp(lr=1e-2, wd=0.01, decay=dec) for dec in (0.0, 0.25, 0.5, 0.999, 1.0)]
    out += [aw_hp(found=f, ema_on_skip=s) for f in (0.0, 1.0) for s in (0, 1)]
    return out


DEFECTS = {                                # name -> the issue's number and wording; _defect_runs applies it to the emulations
    "stale_b": "1 second-trip elements of a grid-stride loop take b from the first trip",
    "swap_coef": "2 coef1 and coef2 swapped",
    "swap_recip": "3 sqrt_recip and sqrt_recipm1 swapped",
    "swap_log": "4 min_log and max_log swapped",
    "frac_unrounded": "5 frac not rounded to the 16-bit dtype in the loss",
    "no_mask": "6 the t = 0 noise mask dropped",
    "no_clip": "7 clip ignored",
    "no_eta": "8 eta ignored",
    "abp_at_t": "9 abar_prev read at t instead of its own row",
    "left_branch_wide": "10 the decoder branch for x0 < -0.999 taken for x0 < 0.999",
    "clamp_grad_live": "11 the clamp gradient left live where arg < 1e-12",
    "no_ln2": "12 vb missing 1 / ln 2",
    "no_range_factor": "13 the v-gradient missing the (max_log - min_log) / 2 factor",
    "swap_g": "14 g_eps and g_v swapped in the backward",
    "bias_before_increment": "15 the AdamW bias correction using the step count before the increment",
    "wd_after": "16 weight decay applied after the update",
    "no_bc2": "17 sqrt(v) not divided by sqrt(bc2)",
    "ema_old_weight": "18 the EMA taking the old weight",
    "one_step_for_all": "19 one tensor's step count used for all tensors",
    "skip_tail": "20 the tail of a tensor (n % 4) skipped",
    "blind_tail": "21 the non-finite check blind to the last sub-vector tail",
    "blind_neg_inf": "22 the non-finite check blind to -Inf",
}


def _defect_runs(name):
    """Every (label, ratio) of the defective emulation on the prescribed cases that the defect can touch."""
    qs = lambda c: qs_eval(c, qs_emul(c, name), strict=False)
    tl = lambda c: tl_eval(c, *tl_emul(c, name), strict=False)
    lb = lambda c: lb_eval(c, lb_emul(c, name), strict=False)
    ds = lambda c: ds_eval(c, *ds_emul(c, name), strict=False)
    aw = lambda hp: aw_eval(_AW, hp, aw_emul(_AW, hp, name), strict=False)
    small_tl = lambda dt: [c for c in tl_cases(dt, big=False) if c.B <= 7 and c.s.spec == ""]
    small_ds = lambda dt: [c for c in ds_cases(dt, big=False) if c.s.spec == ""]
    if name == "stale_b":
        yield "q_sample", qs(qs_cases()[-1])
        yield "loss_bwd", lb(lb_cases(F32)[-1])
        yield "step", ds(ds_cases(F32)[-1])
    elif name in ("swap_coef", "swap_log"):
        for c in small_tl(F32):
            yield "loss", tl(c)
        for c in small_ds(F32):
            yield "step", ds(c)
    elif name == "swap_recip":
        yield "q_sample", qs(qs_cases()[0])
        for c in small_tl(F32):
            yield "loss", tl(c)
        for c in small_ds(F32):
            yield "step", ds(c)
    elif name == "frac_unrounded":
        for dt in (BF16, F16):
            for c in small_tl(dt):
                yield NAME[dt], tl(c)
    elif name in ("left_branch_wide", "clamp_grad_live", "no_ln2", "no_range_factor"):
        for c in small_tl(F32):
            yield "loss", tl(c)
    elif name in ("no_mask", "no_clip", "no_eta", "abp_at_t"):
        for c in small_ds(F32):
            yield "step", ds(c)
    elif name == "swap_g":
        yield "loss_bwd", lb(lb_cases(F32)[0])
    elif name in ("blind_tail", "blind_neg_inf"):
        for pos in nf_positions():
            for val in (INF, -INF, NAN):
                gs = nf_case(pos, val)
                for al in (True, False):
                    yield f"{pos} {val}", nf_eval(gs, nf_emul(gs, al, name), strict=False)
    else:
        for hp in aw_hps():
            yield f"lr {hp.lr} wd {hp.wd} decay {hp.decay}", aw(hp)


_AW = aw_case(seed=5)


# =====================================================================================================================================
# Self-tests
# =====================================================================================================================================
def test_tables_are_permuted_and_padded():
    for spec, T in (("", 1000), ("250", 250)):
        s = schedule(spec)
        assert s.T == T and s.tab.shape == (NROWS, T) and int(s.tab.isnan().all(1).sum()) == NROWS - len(ROWS)
        assert float(s.col["c1"][0]) == pytest.approx(1.0, abs=1e-6) and float(s.col["c2"][0]) == 0.0 and float(s.col["abp"][0]) == 1.0


def test_decoder_inputs_sit_on_their_intended_side():
    """No element of a t = 0 sample is excluded: each is live with arg >= 1e-4 in fp64 (and live in the emulation), or dead with both
    cdfs saturated, val = -log(1e-12) to an ulp and dval == 0 exactly.  All three branches have both populations."""
    seen = False
    for dt in DTYPES:
        for c in tl_cases(dt):
            if not bool(c.is0.any()):
                continue
            nl, nd, br = tl_sides(c)
            if c.per == 3136 and c.B == 3:
                seen = True
                assert nl > 0 and nd > 0 and all(x > 0 for x in br["live"]) and all(x > 0 for x in br["dead"]), br
    assert seen


def test_emulation_meets_every_bound(capsys):
    book = {}
    for c in qs_cases():
        qs_eval(c, qs_emul(c), book)
    for dt in DTYPES:
        for c in tl_cases(dt):
            tl_eval(c, *tl_emul(c), book)
        for c in lb_cases(dt):
            lb_eval(c, lb_emul(c), book)
        for c in ds_cases(dt):
            ds_eval(c, *ds_emul(c), book)
    for hp in aw_hps():
        aw_eval(_AW, hp, aw_emul(_AW, hp), book)
    for pos in [None] + nf_positions():
        for val in (INF, -INF, NAN):
            gs = nf_case(pos, val)
            for al in (True, False):
                nf_eval(gs, nf_emul(gs, al), book)
    with capsys.disabled():
        for k in sorted(book):
            print(f"emulation ratio {k[0]:18s} {k[1]}: {book[k]:.3f}")


def test_out_of_range_timesteps_in_the_emulation():
    for spec in SPECS:
        T = schedule(spec).T
        t = [3, -1, T - 1, T, 0, 2 ** 40, 7]
        c = qs_case(spec, 7, 3, 7, t=t, seed=60)
        out = qs_emul(c)
        assert bool(out[[1, 3, 5]].isnan().all()) and bool(out[[0, 2, 4, 6]].isfinite().all())
        qs_eval(c, out, {})
        c = tl_case(F32, spec, 7, 3, 7, t=t, seed=61)
        tl_eval(c, *tl_emul(c), {})
        c = ds_case(F32, spec, 7, 3, 7, 1, 0.5, 1, t=t, seed=62)
        ds_eval(c, *ds_emul(c), {})
        assert ds_eval(c, *ds_emul(ds_case(F32, spec, 7, 3, 7, 1, 0.5, 1, t=[3, 5, T - 1, 9, 0, 8, 7], seed=62)), strict=False) == INF


@pytest.mark.parametrize("name", list(DEFECTS))
def test_seeded_defect_exceeds_four_times_its_bound(name):
    worst, where = 0.0, None
    for label, r in _defect_runs(name):
        if r > worst:
            worst, where = r, label
        if worst == INF:
            break
    assert worst > 4.0, f"defect {DEFECTS[name]}: largest error / bound {worst} (at {where})"


def test_second_trip_cases_are_second_trip():
    assert qs_cases()[-1].B * qs_cases()[-1].per > GRID
    assert lb_cases(F32)[-1].B * 2 * lb_cases(F32)[-1].per > GRID
    assert all(c.B * c.per > GRID for c in ds_cases(F32)[-2:])
