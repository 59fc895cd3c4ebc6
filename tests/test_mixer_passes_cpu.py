"""The memory-bound passes between the scans and the GEMMs (csrc/merge.hip, csrc/gate_head.hip): the parts that need no GPU.

Input builders, fp64 references, fp32 emulations, bound functions and their self-tests for dm_token_merge (plain, gated, fp32 to
16-bit), dm_gate_bwd, dm_sum_partials, dm_colsum_f32 and dm_gate_head_fwd / dm_gate_head_bwd.  tests/test_mixer_passes_gpu.py
imports all of it and feeds the kernels' outputs to the same `*_eval` functions the emulations go through here.

Inputs are drawn on the host and rounded to their storage dtype first; the reference is plain torch fp64 on those rounded values;
every output is compared per element.

Symbols: u = unit roundoff of the STORED dtype (2^-8 bf16, 2^-11 fp16, 0 fp32); T = the subnormal rounding term (2^-24 fp16, 2^-120
bf16 as an fp32 value cannot get closer to the flush); F = 2^-100, an absolute floor (fp32 denormal results are flushed: silu(-88.7) is
about 1e-37 and comes back as 0); EPS32 = 2^-24.
c(z) = (2|z| + 12) EPS32 is the error of silu_f / sigmoid_f (dm_common.h:316-319): the argument product -z * LOG2E and the rounded
constant move the exponent by up to 2|z| EPS32 relative to e, v_exp_f32 is 1 ulp (2 EPS32), 1 + e one rounding, v_rcp_f32 1 ulp, the
product with z one more, and the rest of the 12 is room for the product that consumes it.  c'(z) = (2|z| + 16) EPS32 is the same with
the four further roundings of silu' = sg (1 + z (1 - sg)) and the products in front of it.

Bounds
  * token_merge sums (merge.hip:45-60): acc starts at 0 and adds the slabs k = 0, 1, 2, ... in fp32, nothing to contract.  `pre` and
    every ungated `out` EQUAL that sequence rounded to nearest even into the output dtype, bit for bit (merge.hip:67, 77).
  * gated out (merge.hip:70-73): ref = base * silu(z), base = the ROUNDED pre if pre is requested and the fp32 sum otherwise;
    |out - ref| <= (u + c(z) (1 + u)) |ref| + T + F.
  * gate_bwd (merge.hip:164-167): g = dy z sg: (u + c(z)) |ref| + T + F.  dz = dy pre sg (1 + z (1 - sg)) cancels near z = -1.278,
    so its fp32 error is relative to the magnitude form: u |ref| (1 + c') + c' |dy pre| sg (1 + |z| (1 - sg)) (1 + u) + T + F.
  * sum_partials (merge.hip:298-302): a sequential fp32 sum of nw rows and one store:
    u |ref| + T + (nw - 1) EPS32 sum_w |in_w|; integer-valued inputs give the exactly rounded sum.
  * colsum (merge.hip:238-253): a wave sums ceil(R / 16) rows, some of them in pairs first, 16 waves meet in LDS:
    (ceil(R / 16) + 20) EPS32 sum_r |x| per column; integer-valued inputs are exact whatever the order (sums stay below 2^24).
  * gate_head_fwd (gate_head.hip:37-53): x = h + b1, s = a per-lane sequential sum of NIT VEC terms then a 6-step wave sum,
    gh_sigmoid = __expf and a true division (gate_head.hip:19).
    E_s = sum_c |silu(x_c) w2_c| ((2|x_c| + 16) EPS32 + (NIT VEC + 8) EPS32);
    |a - ref| <= ref (1 - ref) E_s + (u + (2|s + b2| + 16) EPS32) ref + T + F.
  * gate_head_bwd (gate_head.hip:75-121): `a` is an input and the reference takes the very `a` the test passes.
    dh: u |ref| + c'(x) |dpre w2| sg (1 + |x| (1 - sg)) (1 + u) + T + F.
    part (its nblk rows added in fp64) against the fp64 sums of the UNROUNDED terms: (ceil(rows / (4 nblk)) + 12) EPS32 sum_r |term|
    plus the sum of the terms' own c' error; columns 2C + 1 .. 2C + 3 exactly 0; a workgroup that owns no rows writes a zero row.

The emulations round where the kernels round (torch's accurate exp2 / exp and a correctly rounded division stand in for the 1-ulp
hardware instructions, which the constants 12 and 16 hold).  Largest error-to-bound ratio of the emulation over every input class of
`emulation_cases` (test_emulation_meets_every_bound prints them):
    token_merge   fp32 0.373  bf16 0.992  fp16 0.990        gate_bwd       fp32 0.341  bf16 0.989  fp16 0.988
    sum_partials  fp32 0.994  bf16 0.990  fp16 0.978        colsum         fp32 0.137
    gate_head_fwd fp32 0.086  bf16 0.991  fp16 0.973        gate_head_bwd  fp32 0.276  bf16 0.994  fp16 0.979
(16-bit: nearly all of it is the output's own half-ulp rounding, which the bound charges as u |ref|; sum_partials in fp32 at nw = 2
is ONE rounding against a bound of one rounding.)
"""
import math
from types import SimpleNamespace as NS

import pytest
import torch

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DTYPES = [F32, BF16, F16]
NAME = {F32: "fp32", BF16: "bf16", F16: "fp16"}
CODE = {F32: 0, BF16: 1, F16: 2}
EPS32 = 2.0 ** -24
UNIT = {F32: 0.0, BF16: 2.0 ** -8, F16: 2.0 ** -11}
TINY = {F32: 0.0, BF16: 2.0 ** -120, F16: 2.0 ** -24}
FLOOR = 2.0 ** -100
VECMAX = {F32: 4, BF16: 8, F16: 8}
DM_OK, DM_ERR_ARG, DM_ERR_LAYOUT, DM_ERR_DTYPE = 0, -1, -2, -3
NAN = float("nan")
LOG2E = 1.4426950408889634
Z_EDGES = [0.0, -0.0, 30.0, -30.0, 60.0, -60.0, 100.0, -100.0, -1.278, -1.2785]

RATIOS = {}            # (operator, dtype name) -> largest error / bound the GPU file has seen


def c_z(z):
    return (2 * z.abs() + 12) * EPS32


def c_p(z):
    return (2 * z.abs() + 16) * EPS32


def rnd(x, dt):
    """fp32 -> dt, round to nearest even (what io<T>::st does)."""
    return x.to(dt)


def trunc(x, dt):
    """fp32 -> dt, rounded toward zero (a defect)."""
    if dt == F32:
        return x.clone()
    if dt == BF16:
        return (x.contiguous().view(torch.int32) & -65536).view(F32).to(BF16)
    r = x.to(F16)
    over = (r.float().abs() > x.abs()).to(torch.int16)
    return (r.view(torch.int16) - over).view(F16)


def bits_equal(a, b):
    it = {4: torch.int32, 2: torch.int16}[a.element_size()]
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it))


def check(op, dt, name, got, ref, tol, book=None):
    """Per-element |got - ref| <= tol (NaN in got -- an element the kernel never wrote -- fails); returns and records the largest
    error-to-bound ratio."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, f"{op} {name}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    tol = torch.as_tensor(tol, dtype=torch.float64).expand_as(ref)
    err = (got - ref).abs()
    bad = ~(err <= tol)
    if bool(bad.any()):
        i = int(bad.flatten().nonzero()[0])
        raise AssertionError(f"{op} {NAME[dt]} {name}: {int(bad.sum())} of {ref.numel()} elements out of bound; first at flat {i}: "
                             f"got {float(got.flatten()[i])} ref {float(ref.flatten()[i])} tol {float(tol.flatten()[i])}")
    ratio = float(torch.where(err == 0, torch.zeros_like(err), err / tol).max()) if ref.numel() else 0.0
    book = RATIOS if book is None else book
    book[(op, NAME[dt])] = max(book.get((op, NAME[dt]), 0.0), ratio)
    return ratio


def exact(op, dt, name, got, want, book=None):
    if not bits_equal(got, want):
        g, w = got.detach().cpu().double().flatten(), want.double().flatten()
        bad = ~((g == w) | (g.isnan() & w.isnan()))
        i = int(bad.nonzero()[0]) if bool(bad.any()) else 0
        raise AssertionError(f"{op} {NAME[dt]} {name}: not the exactly rounded result; {int(bad.sum())} of {w.numel()} differ, first at "
                             f"flat {i}: got {float(g[i])} want {float(w[i])}")
    book = RATIOS if book is None else book
    book.setdefault((op, NAME[dt]), 0.0)


def sig32(z):
    """sigmoid_f (dm_common.h:316-318) in fp32."""
    return 1.0 / (1.0 + torch.exp2(-z * torch.tensor(LOG2E, dtype=F32)))


def gh_sig32(x):
    """gh_sigmoid (gate_head.hip:19) in fp32."""
    return 1.0 / (1.0 + torch.exp(-x))


def z_values(shape, g):
    """Gate values: 3 N(0, 1) with the edges (0, -0.0, +-30, +-60, +-100, the zero of silu') and a dense band around -1.278 in front."""
    n = math.prod(shape)
    z = 3 * torch.randn(n, generator=g, dtype=torch.float64)
    e = torch.tensor(Z_EDGES, dtype=torch.float64)[:n]
    z[:e.numel()] = e
    m = min(64, max(0, (n - e.numel()) // 2))
    z[e.numel():e.numel() + m] = torch.linspace(-1.4, -1.15, m, dtype=torch.float64) if m else z[:0]
    return z.view(shape)


# =====================================================================================================================================
# dm_token_merge
# =====================================================================================================================================
def merge_case(dt, B, L, D, K, *, values="randn", table=None, gated=False, want_pre=False, out_dt=None, seed=0):
    """slabs [K, B, L, D] in dt, the row tables [K, L] (gather: out[t] = sum_k in[k][idx[k][t]]), the gate z [B, L, D]."""
    g = torch.Generator().manual_seed(seed)
    idx = None
    if table == "identity":
        idx = torch.arange(L).repeat(K, 1)
    elif table == "perm":
        idx = torch.stack([torch.randperm(L, generator=g) for _ in range(K)])
    elif table == "repeat":
        idx = torch.randint(0, L, (K, L), generator=g)
        idx[:, -1] = idx[:, 0]
    v = torch.randn(K, B, L, D, generator=g, dtype=torch.float64)
    if values == "sub16":                                   # fp16 subnormals (below 2^-14)
        v = v * 2.0 ** -19
    v = v.to(dt)
    if values == "cancel":                                  # s1 = -s0 and a small s2: the fp32 sequence returns s2 exactly
        assert K >= 3 and table != "repeat"
        v[1] = -v[0]
        v[2] = (1e-3 * v[2].double()).to(dt)
        v[3:] = 0
        if idx is not None:                                 # v holds the gathered rows: place them where the tables look
            s = torch.empty_like(v)
            for k in range(K):
                s[k][:, idx[k]] = v[k]
            v = s
    z = z_values((B, L, D), g).to(dt) if gated else None
    return NS(dt=dt, out_dt=out_dt or dt, B=B, L=L, D=D, K=K, slabs=v, idx=None if idx is None else idx.to(torch.int32), z=z,
              gated=gated, want_pre=gated and want_pre)


def merge_expected(c):
    acc = torch.zeros(c.B, c.L, c.D, dtype=F32)
    for k in range(c.K):
        s = c.slabs[k].float()
        acc = acc + (s if c.idx is None else s[:, c.idx[k].long()])
    return acc


def merge_emul(c, defect=None):
    """(out, pre) as merge_kernel computes them; `defect` names one seeded fault."""
    st = trunc if defect == "truncate" else rnd
    acc = torch.zeros(c.B, c.L, c.D, dtype=F32)
    for k in range(c.K):
        s = c.slabs[k].float()
        if c.idx is not None:
            i = c.idx[k].long()
            if defect == "scatter":
                t = torch.zeros_like(s)
                t[:, i] = s
                s = t
            else:
                s = s[:, i]
        acc = acc + s
        if defect == "sum_in_io":
            acc = acc.to(c.dt).float()
    pre = None
    if c.gated:
        z = c.z.float()
        if defect == "gate_via_index" and c.idx is not None:
            z = z[:, c.idx[c.K - 1].long()]
        if c.want_pre:
            pre = st(acc, c.dt)
            if defect != "gate_unrounded":
                acc = pre.float()
        acc = acc * (z * sig32(z))
    out = st(acc, c.out_dt)
    if defect == "drop_tail":                               # the last partial vector of a row never written
        n = (c.D // VECMAX[c.dt]) * VECMAX[c.dt]
        out[..., n:] = NAN
        if pre is not None:
            pre[..., n:] = NAN
    return out, pre


def merge_eval(c, out, pre, book=None, op="token_merge"):
    acc = merge_expected(c)
    if c.want_pre:
        exact(op, c.dt, "pre", pre, acc.to(c.dt), book)
    if not c.gated:
        exact(op, c.out_dt, "out", out, acc.to(c.out_dt), book)
        return 0.0
    base = acc.to(c.dt).double() if c.want_pre else acc.double()
    z = c.z.double()
    ref = base * z * torch.sigmoid(z)
    u = UNIT[c.dt]
    return check(op, c.dt, "out", out, ref, (u + c_z(z) * (1 + u)) * ref.abs() + TINY[c.dt] + FLOOR, book)


# =====================================================================================================================================
# dm_gate_bwd
# =====================================================================================================================================
def gate_bwd_case(dt, B, L, D, seed=0):
    """z over its value classes, pre and dy at magnitudes 1e-3 .. 1e3 (fp16: dy scaled down where a result would leave the format)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda: torch.randn(B, L, D, generator=g, dtype=torch.float64)
    mag = lambda: 10.0 ** (6 * torch.rand(B, L, D, generator=g, dtype=torch.float64) - 3)
    z = z_values((B, L, D), g).to(dt)
    pre = (rn() * mag()).to(dt)
    dy = rn() * mag()
    if dt == F16:
        dy = dy * (1e4 / (dy.abs() * (1 + z.double().abs()) * pre.double().abs().clamp_min(1))).clamp_max(1)
    return NS(dt=dt, B=B, L=L, D=D, z=z, pre=pre, dy=dy.to(dt))


def gate_bwd_emul(c, defect=None):
    dy, z, pre = c.dy.float(), c.z.float(), c.pre.float()
    sg = sig32(z)
    g = dy * z * sg
    dz = dy * pre * sg if defect == "no_z_term" else dy * pre * sg * (1.0 + z * (1.0 - sg))
    if defect == "swapped":
        g, dz = dz, g
    return rnd(g, c.dt), rnd(dz, c.dt)


def gate_bwd_eval(c, g, dz, book=None, op="gate_bwd"):
    dy, z, pre = c.dy.double(), c.z.double(), c.pre.double()
    sg = torch.sigmoid(z)
    u, T = UNIT[c.dt], TINY[c.dt]
    ref_g = dy * z * sg
    r1 = check(op, c.dt, "g", g, ref_g, (u + c_z(z)) * ref_g.abs() + T + FLOOR, book)
    ref_dz = dy * pre * sg * (1 + z * (1 - sg))
    cp = c_p(z)
    tol = u * ref_dz.abs() * (1 + cp) + cp * (dy * pre).abs() * sg * (1 + z.abs() * (1 - sg)) * (1 + u) + T + FLOOR
    return max(r1, check(op, c.dt, "dz", dz, ref_dz, tol, book))


# =====================================================================================================================================
# dm_sum_partials / dm_colsum_f32
# =====================================================================================================================================
def int_grid(*shape, mod=61):
    """Integer values that are a function of every index, so that a dropped, doubled or exchanged row or column shows."""
    n = torch.zeros(shape, dtype=torch.int64)
    for d, (s, p) in enumerate(zip(shape, (131, 29, 7, 3))):
        n = n + (torch.arange(s) * p).view([-1 if i == d else 1 for i in range(len(shape))])
    i0 = torch.arange(shape[0]).view([-1] + [1] * (len(shape) - 1))
    i1 = torch.arange(shape[-1]).view([1] * (len(shape) - 1) + [-1])
    return ((n + (i0 * i1) % 7) % mod - mod // 2).float()


def sum_partials_case(dt, rows, nw, cols, integer, seed=0):
    if integer:
        x = int_grid(rows, nw, cols)
    else:
        g = torch.Generator().manual_seed(seed)
        x = torch.randn(rows, nw, cols, generator=g) * 10.0 ** (2 * torch.rand(rows, nw, cols, generator=g) - 1)
    return NS(dt=dt, rows=rows, nw=nw, cols=cols, x=x, integer=integer)


def sum_partials_emul(c, defect=None):
    acc = c.x[:, 0].clone()
    for w in range(1, c.nw):
        if defect == "skip_row" and w == c.nw - 1:
            continue
        acc = acc + c.x[:, w]
    return rnd(acc, c.dt)


def sum_partials_eval(c, out, book=None, op="sum_partials"):
    ref = c.x.double().sum(1)
    if c.integer:
        exact(op, c.dt, "out", out, ref.to(c.dt), book)
        return 0.0
    tol = UNIT[c.dt] * ref.abs() + TINY[c.dt] + (c.nw - 1) * EPS32 * c.x.double().abs().sum(1)
    return check(op, c.dt, "out", out, ref, tol, book)


def colsum_case(R, C, integer, seed=0):
    if integer:
        return int_grid(R, C, mod=201)
    g = torch.Generator().manual_seed(seed)
    return torch.randn(R, C, generator=g) * 10.0 ** (2 * torch.rand(R, C, generator=g) - 1)


def colsum_emul(x):
    """The summation order of colsum_kernel (merge.hip:238-253)."""
    R, C = x.shape
    tot = torch.zeros(C, dtype=F32)
    for w in range(16):
        acc = torch.zeros(C, dtype=F32)
        r = w
        while r + 48 < R:
            acc = acc + ((x[r] + x[r + 16]) + (x[r + 32] + x[r + 48]))
            r += 64
        while r < R:
            acc = acc + x[r]
            r += 16
        tot = tot + acc
    return tot


def colsum_eval(x, out, integer, book=None, op="colsum"):
    ref = x.double().sum(0)
    if integer:
        exact(op, F32, "out", out, ref.float(), book)
        return 0.0
    R = x.shape[0]
    return check(op, F32, "out", out, ref, (math.ceil(R / 16) + 20) * EPS32 * x.double().abs().sum(0) + FLOOR, book)


# =====================================================================================================================================
# dm_gate_head_fwd / dm_gate_head_bwd
# =====================================================================================================================================
def gh_nit(dt, C):
    need = -(-C // (64 * VECMAX[dt]))
    return 1 if need <= 1 else 2 if need <= 2 else 4


def _saturate(x_row, w2, b1, b2, target):
    """A row x_c = sign * sign(w2_c) * v with v bisected (fp64) so that sum_c silu(x_c) w2_c + b2 is about `target`."""
    sgn = 1.0 if target > 0 else -1.0
    d = torch.where(w2 >= 0, 1.0, -1.0).double() * sgn
    f = lambda v: float((torch.nn.functional.silu(d * v) * w2.double()).sum()) + b2
    lo, hi = 1.3, 400.0
    if (f(hi) - target) * sgn < 0:
        return x_row                                        # every w2 of one sign: this width cannot reach the target
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if (f(mid) - target) * sgn < 0:
            lo = mid
        else:
            hi = mid
    return d * hi


def gh_case(dt, R, C, seed=0, has_b1=True, has_b2=True):
    """h [R, C] in dt with x = h + b1 over its value classes: +-30 / +-100 sprinkled into every third row, row 1 a dense band around
    -1.278, rows 2 and 3 with s + b2 near +20 and -20 (a = 1 / 0 after rounding), the rest 2 N(0, 1).  For the backward `a` is the
    rounded fp64 forward with rows 4 and 5 set to exactly 0 and 1, and da is N(0, 1)."""
    g = torch.Generator().manual_seed(seed)
    w2 = (2.0 / math.sqrt(C)) * torch.randn(C, generator=g)
    b1 = 0.5 * torch.randn(C, generator=g) if has_b1 else None
    b2 = torch.tensor([0.25]) if has_b2 else None
    x = 2 * torch.randn(R, C, generator=g, dtype=torch.float64)
    edges = torch.tensor([30.0, -30.0, 100.0, -100.0], dtype=torch.float64)
    for r in range(0, R, 3):
        x[r, (r // 3) % C] = edges[(r // 3) % 4]
    if R > 1:
        x[1] = torch.linspace(-1.4, -1.15, C, dtype=torch.float64)
    b2v = 0.25 if has_b2 else 0.0
    if R > 3:
        x[2] = _saturate(x[2], w2, b1, b2v, 20.0)
        x[3] = _saturate(x[3], w2, b1, b2v, -20.0)
    h = (x - (b1.double() if has_b1 else 0.0)).to(dt)
    c = NS(dt=dt, R=R, C=C, h=h, b1=b1, w2=w2, b2=b2, nit=gh_nit(dt, C))
    a = gh_fwd_ref(c)[0].to(dt)
    if R > 5:
        a[4], a[5] = 0.0, 1.0
    c.a, c.da = a, torch.randn(R, generator=g).to(dt)
    return c


def _gh_x64(c):
    return c.h.double() + (c.b1.double() if c.b1 is not None else 0.0)


def gh_fwd_ref(c):
    x = _gh_x64(c)
    term = torch.nn.functional.silu(x) * c.w2.double()
    sb = term.sum(1) + (float(c.b2) if c.b2 is not None else 0.0)
    return torch.sigmoid(sb), sb, x, term


def gh_fwd_emul(c, defect=None, store=True):
    VEC, NIT = VECMAX[c.dt], c.nit
    w2 = c.w2
    b1 = c.b1 if c.b1 is not None else torch.zeros(c.C)
    if defect == "b1_after_silu":
        h = c.h.float()
        t = (h * gh_sig32(h) + b1) * w2
    else:
        x = c.h.float() + b1
        t = x * gh_sig32(x) * w2
    pad = torch.zeros(c.R, NIT * 64 * VEC, dtype=F32)
    pad[:, :c.C] = t
    lanes = pad.view(c.R, NIT, 64, VEC).permute(0, 2, 1, 3).reshape(c.R, 64, NIT * VEC)
    s = torch.zeros(c.R, 64, dtype=F32)
    for i in range(NIT * VEC):
        s = s + lanes[..., i]
    n = 64
    while n > 1:
        n //= 2
        s = s[:, :n] + s[:, n:]
    s = s[:, 0]
    if c.b2 is not None and defect != "no_b2":
        s = s + c.b2.float()
    a = gh_sig32(s)
    if store:
        a = rnd(a, c.dt)
    if defect == "first_trip_only":                         # the rows past the first grid-stride trip (4096 workgroups x 4 waves)
        a[4 * 4096:] = NAN
    return a


def gh_fwd_eval(c, a, book=None, op="gate_head_fwd"):
    ref, sb, x, term = gh_fwd_ref(c)
    E_s = (term.abs() * ((2 * x.abs() + 16) * EPS32 + (c.nit * VECMAX[c.dt] + 8) * EPS32)).sum(1)
    tol = ref * (1 - ref) * E_s + (UNIT[c.dt] + (2 * sb.abs() + 16) * EPS32) * ref + TINY[c.dt] + FLOOR
    return check(op, c.dt, "a", a, ref, tol, book)


def gh_bwd_emul(c, nblk, defect=None):
    """(dh, part) as gate_head_bwd_kernel computes them: rows dealt round-robin to 4 nblk waves, four waves meet in LDS."""
    R, C = c.R, c.C
    x = c.h.float() + (c.b1 if c.b1 is not None else torch.zeros(C))
    sg = gh_sig32(x)
    a = gh_fwd_emul(c, store=False) if defect == "dpre_unrounded_a" else c.a.float()
    dpre = c.da.float() * a * (1.0 - a)
    sp = sg * (1.0 + x * (1.0 - sg))
    gg = dpre[:, None] * c.w2 * sp
    t2 = dpre[:, None] * sp if defect == "dw2_silu_prime" else dpre[:, None] * x * sg
    dh = rnd(gg, c.dt)
    nwv = 4 * nblk
    acc = torch.zeros(nwv, 2 * C + 1, dtype=F32)
    for r in range(R):
        if defect == "first_trip_only" and r >= nwv:
            dh[r] = NAN
            continue
        acc[r % nwv] = acc[r % nwv] + torch.cat([gg[r], t2[r], dpre[r:r + 1]])
    part = torch.zeros(nblk, 2 * C + 4, dtype=F32)
    for b in range(nblk):
        s = torch.zeros(2 * C + 1, dtype=F32)
        for w in range(4):
            s = s + acc[4 * b + w]
        part[b, :2 * C + 1] = s
    return dh, part


def gh_bwd_eval(c, dh, part, nblk, book=None, op="gate_head_bwd"):
    R, C = c.R, c.C
    u, T = UNIT[c.dt], TINY[c.dt]
    x = _gh_x64(c)
    sg = torch.sigmoid(x)
    a = c.a.double()
    dpre = (c.da.double() * a * (1 - a))[:, None]
    w2 = c.w2.double()
    ref = dpre * w2 * sg * (1 + x * (1 - sg))
    cp = c_p(x)
    mag = (dpre * w2).abs() * sg * (1 + x.abs() * (1 - sg))
    r = check(op, c.dt, "dh", dh, ref, u * ref.abs() + cp * mag * (1 + u) + T + FLOOR, book)
    part = part.detach().cpu()
    assert tuple(part.shape) == (nblk, 2 * C + 4)
    assert bool((part[:, 2 * C + 1:] == 0).all()), f"{op}: part columns 2C+1 .. 2C+3 must be exactly 0"
    for b in range(nblk):
        if 4 * b >= R:
            assert bool((part[b] == 0).all()), f"{op}: workgroup {b} owns no rows and must write a zero partial row"
    p = part.double().sum(0)
    gr = (math.ceil(R / (4 * nblk)) + 12) * EPS32
    t2 = dpre * x * sg
    r = max(r, check(op, c.dt, "part.db1", p[:C], ref.sum(0), gr * ref.abs().sum(0) + (cp * mag).sum(0) + FLOOR, book))
    r = max(r, check(op, c.dt, "part.dw2", p[C:2 * C], t2.sum(0), gr * t2.abs().sum(0) + (cp * t2.abs()).sum(0) + FLOOR, book))
    sd = dpre.abs().sum()
    return max(r, check(op, c.dt, "part.db2", p[2 * C], dpre.sum(), gr * sd + 16 * EPS32 * sd + FLOOR, book))


# =====================================================================================================================================
# the input classes both files run, and the self-tests
# =====================================================================================================================================
MERGE_DEFECTS = ["gate_unrounded", "gate_via_index", "scatter", "truncate", "drop_tail", "sum_in_io"]
GATE_BWD_DEFECTS = ["no_z_term", "swapped"]
GH_FWD_DEFECTS = ["b1_after_silu", "no_b2", "first_trip_only"]
GH_BWD_DEFECTS = ["dw2_silu_prime", "first_trip_only", "dpre_unrounded_a"]


def merge_cases(dt):
    """The value and table classes of dm_token_merge at the small shapes of the GPU file (the alignment classes reuse them)."""
    cs = []
    for D in (1, 7, 8, 263):
        cs.append(merge_case(dt, 2, 5, D, 3, seed=D))
        cs.append(merge_case(dt, 2, 5, D, 3, gated=True, want_pre=True, table="perm", seed=100 + D))
        cs.append(merge_case(dt, 2, 5, D, 3, gated=True, table="perm", seed=200 + D))
    for K in (1, 2, 3, 4):
        for table in (None, "identity", "perm", "repeat"):
            cs.append(merge_case(dt, 2, 5, 24, K, table=table, seed=300 + K))
            cs.append(merge_case(dt, 2, 5, 24, K, table=table, gated=True, want_pre=K % 2 == 1, seed=400 + K))
    for table in (None, "perm"):
        cs.append(merge_case(dt, 2, 5, 40, 3, values="cancel", table=table, seed=500))
        cs.append(merge_case(dt, 2, 5, 40, 4, values="cancel", table=table, gated=True, want_pre=True, seed=501))
    cs.append(merge_case(dt, 2, 5, 40, 3, values="sub16", seed=502))
    cs.append(merge_case(dt, 2, 5, 40, 3, values="sub16", gated=True, want_pre=True, seed=503))
    if dt == F32:
        for o in (BF16, F16):
            cs.append(merge_case(F32, 2, 5, 24, 3, out_dt=o, table="perm", seed=600))
            cs.append(merge_case(F32, 2, 5, 7, 2, out_dt=o, seed=601))
            cs.append(merge_case(F32, 2, 5, 40, 3, out_dt=o, values="sub16", seed=602))
    return cs


def gate_bwd_cases(dt):
    return [gate_bwd_case(dt, 2, 5, D, seed=700 + D) for D in (1, 7, 8, 263)] + [gate_bwd_case(dt, 1, 3, 8 * 257, seed=710)]


def sum_partials_cases(dt):
    cs = []
    for integer in (True, False):
        for rows, nw, cols in [(37, 2, 32), (1, 7, 36), (5, 16, 4), (5, 1, 256), (37, 7, 36), (1, 16, 256)]:
            cs.append(sum_partials_case(dt, rows, nw, cols, integer, seed=800 + rows + nw))
    return cs


COLSUM_R = [1, 2, 15, 16, 17, 63, 64, 65, 79, 80, 81, 129]
COLSUM_C = [4, 252, 256, 260, 516]
GH_WIDTHS = {F32: [4, 252, 256, 260, 512, 516, 1020, 1024], BF16: [8, 504, 512, 520, 1024, 1032, 2040, 2048],
             F16: [8, 504, 512, 520, 1024, 1032, 2040, 2048]}
GH_NBLK = [(1, 37), (3, 29), (8, 5)]                        # (nblk, rows): one workgroup walks all rows; rows do not divide the waves;
                                                            # more workgroups than rows


def gh_cases(dt):
    cs = [gh_case(dt, 9, C, seed=900 + C) for C in GH_WIDTHS[dt]]
    cs.append(gh_case(dt, 9, 64, seed=990, has_b1=False))
    cs.append(gh_case(dt, 9, 64, seed=991, has_b2=False))
    return cs


def test_emulation_meets_every_bound():
    """The fp32 emulation of each operator, rounding where the kernel rounds, is inside every bound on every input class."""
    book = {}
    for dt in DTYPES:
        for c in merge_cases(dt):
            merge_eval(c, *merge_emul(c), book=book)
        for c in gate_bwd_cases(dt):
            gate_bwd_eval(c, *gate_bwd_emul(c), book=book)
        for c in sum_partials_cases(dt):
            sum_partials_eval(c, sum_partials_emul(c), book=book)
        for c in gh_cases(dt):
            gh_fwd_eval(c, gh_fwd_emul(c), book=book)
            gh_bwd_eval(c, *gh_bwd_emul(c, 2), 2, book=book)
        for nblk, rows in GH_NBLK:
            c = gh_case(dt, rows, 64, seed=950 + nblk)
            gh_bwd_eval(c, *gh_bwd_emul(c, nblk), nblk, book=book)
        c = gh_case(dt, 4 * 4096 + 5, VECMAX[dt], seed=960)
        gh_fwd_eval(c, gh_fwd_emul(c), book=book)
    for R in COLSUM_R + [768]:
        for C in (4, 260):
            for integer in (True, False):
                x = colsum_case(R, C, integer, seed=R)
                colsum_eval(x, colsum_emul(x), integer, book=book)
    for k in sorted(book):
        print(f"emulation {k[0]:14s} {k[1]}: {book[k]:.3f}")
    assert all(v <= 1.0 for v in book.values())
    assert len(book) == 5 * 3 + 1


def _fails(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("defect", MERGE_DEFECTS)
def test_merge_defects_are_told_apart(defect):
    """Each seeded defect of the merge fails on at least one prescribed input (and the clean emulation passes all of them)."""
    hit = 0
    for dt in DTYPES:
        for c in merge_cases(dt):
            merge_eval(c, *merge_emul(c), book={})
            hit += _fails(lambda: merge_eval(c, *merge_emul(c, defect), book={}))
    assert hit > 0, f"no input class separates the defect {defect} from the reference"


@pytest.mark.parametrize("defect", GATE_BWD_DEFECTS)
@pytest.mark.parametrize("dt", DTYPES, ids=list(NAME.values()))
def test_gate_bwd_defects_are_told_apart(dt, defect):
    hit = sum(_fails(lambda: gate_bwd_eval(c, *gate_bwd_emul(c, defect), book={})) for c in gate_bwd_cases(dt))
    assert hit > 0, f"no input class separates the defect {defect} from the reference"


@pytest.mark.parametrize("dt", DTYPES, ids=list(NAME.values()))
def test_sum_partials_defect_is_told_apart(dt):
    for c in sum_partials_cases(dt):
        if c.nw > 1:
            assert _fails(lambda: sum_partials_eval(c, sum_partials_emul(c, "skip_row"), book={})), (c.rows, c.nw, c.cols, c.integer)


@pytest.mark.parametrize("defect", GH_FWD_DEFECTS)
@pytest.mark.parametrize("dt", DTYPES, ids=list(NAME.values()))
def test_gate_head_fwd_defects_are_told_apart(dt, defect):
    cs = [gh_case(dt, 4 * 4096 + 5, VECMAX[dt], seed=960)] if defect == "first_trip_only" else gh_cases(dt)
    hit = sum(_fails(lambda: gh_fwd_eval(c, gh_fwd_emul(c, defect), book={})) for c in cs)
    assert hit > (0 if defect != "b1_after_silu" else 1), f"no input class separates the defect {defect} from the reference"


@pytest.mark.parametrize("defect", GH_BWD_DEFECTS)
@pytest.mark.parametrize("dt", DTYPES, ids=list(NAME.values()))
def test_gate_head_bwd_defects_are_told_apart(dt, defect):
    if defect == "dpre_unrounded_a" and dt == F32:
        return                                              # fp32 stores `a` unrounded: there is no such defect to tell apart
    hit = 0
    for nblk, rows in GH_NBLK[:2]:
        c = gh_case(dt, rows, 64, seed=950 + nblk)
        hit += _fails(lambda: gh_bwd_eval(c, *gh_bwd_emul(c, nblk, defect), nblk, book={}))
    assert hit > 0, f"no input class separates the defect {defect} from the reference"


def test_colsum_emulation_order_and_int_grid():
    """The integer grid tells a dropped row, a doubled row and two exchanged columns from the reference."""
    x = colsum_case(81, 260, True)
    good = colsum_emul(x)
    colsum_eval(x, good, True, book={})
    assert _fails(lambda: colsum_eval(x, good - x[80], True, book={}))
    assert _fails(lambda: colsum_eval(x, good + x[17], True, book={}))
    swapped = good.clone()
    swapped[[3, 4]] = good[[4, 3]]
    assert _fails(lambda: colsum_eval(x, swapped, True, book={}))
