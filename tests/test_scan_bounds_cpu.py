"""The selective scans (K1 scan_fwd_impl.h, K1c scan_fwd_chunked.h, K2 scan_bwd_impl.h, K2c scan_bwd_chunked.h) per element against fp64:
the analysis (reference, closed form, emulation, bounds, defect catalogue), its own CPU tests, and the dm_selective_scan_bwd refusal of
ngroups != 1.  tests/test_scan_bounds_gpu.py imports the analysis and holds the kernels to it.

REFERENCE.  oracle.mamba_ref.selective_scan_ref and fp64 autograd through it, on the inputs as rounded to the I/O dtype.  `manual` restates
forward and backward step by step after the header of csrc/scan_bwd_step.h:6-19 (h_k for k = 0..L; reverse: lambda = C gy + carry, carry =
a lambda, Gt = carry h_{k-1}; dC = h_k gy, dB = lambda dt u, dA += Gt dt, dlA = sum_n A Gt, GB = sum_n lambda B, ddelta = (u GB + dlA) sp',
du = dt GB + gy D, dz = g (C.h_k + D u) silu'(z), dD += gy u, dbias += ddelta) and is pinned to autograd at 1e-12 max|ref| per output for
every call pattern (test_manual_equals_autograd).  The device tests compare with `manual(case)`, i.e. with that reference.
Delta mode 2 (delta holds softplus(raw + bias) already): the reference takes raw + bias = softplus^-1(delta) in fp64 as its leaf.

WHERE THE KERNELS ROUND (u = 2^-8 bf16, 2^-11 fp16, 2^-24 fp32; T = the subnormal step of the format), and nowhere else:
  F1  forward out: D u and the gate in fp32, one store rounding (scan_fwd_impl.h:68-72, :242; chunked the same step).
  F2  accumulating launches (DM_FLAG_OUT_ACCUMULATE): y += old; store -- one rounding per direction of the running sum (scan_fwd_impl.h:241-242).
  F3  checkpoints: the fp32 state after every 4th step, v_cvt_pk_bf16_f32 for bf16 I/O (scan_fwd_impl.h:155-160), fp32 otherwise (:163-166);
      slot 0 = the state after the last step (:284); last_state fp32 (:286-292).
  B1  the states of the sweep: the state after k steps is the stored checkpoint when k % 4 == 0 (slot 0 for k == L: scan_bwd_step.h:124-127,
      scan_bwd_impl.h:409-415), else recomputed in fp32 from the checkpoint entering its sub-chunk (scan_bwd_impl.h:399-408).  With L % 4 != 0
      the last sub-chunk starts from its entering checkpoint and its steps past L meet g = 0 (scan_bwd_impl.h:363-367).
  B2  dB / dC with bf16 I/O: the per-channel products are rounded to bf16 (pack_bf16, scan_bwd_impl.h:465-467; scan_bwd_step.h:152-154) before
      the lane-group sum -- K2 at d_state 8 / 16 / 32 (MFMA_RED, scan_bwd_impl.h:106) and K2c (scan_bwd_chunked.h:59); d_state 64 / 128 and every
      fp16 / fp32 instantiation sum in fp32 (lane_group_reduce, scan_bwd_impl.h:498).
  B3  du, ddelta, dz: one rounding to the I/O dtype (st_cv, scan_bwd_impl.h:484-488).  dB / dC: fp32 partial rows, summed by dm_sum_partials
      into the dtype the caller asks for (fp32 here: hip_ops.scan_bwd).
  B4  dA, dD, dbias leave as fp32 partials per sequence (scan_bwd_impl.h:514-525) and are column-summed in fp32.

BOUNDS, per element, first order plus the products of two errors, all in fp64.  e = 2^-24.  Every line is a count of fp32 operations in the code.
  dt    mode 0: x = raw + bias, one add: |d dt| <= e |x|.  mode 2: dt is an input: 0.  mode 1 (softplus_f, dm_common.h:313-319), s = sigmoid(x):
        x > 20: e |x|.   series (E = e^x < 2^-12):  dt e (3|x| + 7): the add (|x|), the product x LOG2E and the constant (2|x|), v_exp (2), the
        series' truncation E^2/3 < e (1) and its three operations (3), one spare.   else: e (s (3|x| + 2) + 1 + 4 dt): the same |x| terms and
        v_exp through d log(1+E) = s dE/E, the rounding of 1 + E (absolute e on the logarithm: the cancellation that costs small dt its digits),
        v_log (2 dt), the product with LN2 and the constant (2 dt).
  a     a = exp2((A LOG2E) dt): relative e (2 + DK |A| dt) + |A| |d dt|: v_exp 2; the argument's three roundings (constant, A LOG2E, times dt), DK = 3.
        The chunk-parallel kernels fold whole chunks with P = exp2(A2 sum dt) (scan_fwd_chunked.h:9-10, scan_bwd_chunked.h:170-194, :208-217): the
        running sum of up to LC = 28 steps adds LC roundings to the argument, so DK = LC + 3 = 31 for K1c / K2c, charged on every step.
  h     F_k = a F_{k-1} + e (a habs_{k-1} (DK |A| dt + 4) + 4 |b|) + |d dt| (|A| a habs_{k-1} + |B u|) + tiny (1 + habs):  habs_k = a habs_{k-1} + |B dt u|
        (the S-form); 4 = v_exp 2 + the product a h + the final add; 4 |b| = dt u, B (dt u), the final add, one spare; tiny = 2^-126 (flushed results).
        Sweep states: E_k = F_k + ck_k, ck_k = u (|h_k| + F_k) + T at a bf16 checkpoint, a ck_{k-1} after it (sharper than u habs and the same
        places: through |gy| to dC, through |g silu'(z)| sum_n |C| to dz, through the carry to ddelta and dA; not to du or dB).
  gy    g z sigmoid(z) (scan_bwd_step.h:93-99; sigmoid_f dm_common.h:320): relative e CG, CG = 7 + 2|z|: argument 2|z|, v_exp 2, the add 1, v_rcp 2,
        two products.  Without z: exact.
  lam   labs = |C||gy| + cabs, cabs = a labs (S-form).  lerr = |C gy| e (CG + 1) + e labs + cerr;  cerr' = a lerr + a labs (e (3 + DK |A| dt) + |A||d dt|).
  sums  a sum of n fp32 terms in any order: n e sum|terms|.  n = N + 2 for the sums over the states (N terms, the slice_sum adds of the split
        forms, the products), Dm for dB / dC (lane groups, row positions, waves, workgroups, dm_sum_partials), L + S for dA / dD / dbias.
  sp'   1 - exp2(-dt LOG2E) (scan_bwd_step.h:113): absolute e (2 + 2 dt + sp') + |d dt| -- the subtraction is exact, v_exp's error is absolute
        near 1: channels with dt = e^-12 lose 2^-24 / 6e-6 of ddelta here.  Mode 0: the factor is 1.
  f     1 + z (1 - sz) (scan_bwd_step.h:117-119): absolute e (|z| (6 + 2|z|) + 2); dz = g ypre sz f.
  Every stored 16-bit value: + u (|v| + err) + T.  fp16 needs T: small dz / ddelta fall under 2^-14.
No constant, factor or floor is taken from a measured device error.

DEFECTS: `DEFECTS` below names, for each, the outputs and cases that must show > 4 x bound (test_defects_exceed_the_bound).
"""
import ctypes
import functools
import math
from collections import namedtuple

import pytest
import torch

from tests.test_ssd_gpu import EPS32, TINY as _TINY16, UNIT as _UNIT16

BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
NAME = {BF16: "bf16", F16: "f16", F32: "f32"}
TINY32 = 2.0 ** -126
UNIT = {**_UNIT16, F32: EPS32}                                          # 2^-8, 2^-11 as in tests/test_ssd_gpu.py; fp32 I/O through the same bound
TINY = {**_TINY16, F32: TINY32}
SUB = 4                                                                 # DM_SCAN_CKPT_EVERY
WORST = {}

Case = namedtuple("Case", "fam dtype L Dm N ndir bpd mode z tables dps ash bcf32 groups acc ckpt seed")


def case(fam, dtype, L, Dm, N=16, ndir=1, bpd=1, mode=1, z=True, tables=False, dps=False, ash=False, bcf32=False, groups=1, acc=False,
         ckpt=True, seed=0):
    """fam: 'K1' | 'K1c' | 'K2' | 'K2c'.  mode: delta mode 0 / 1 / 2.  tables: two random row tables per direction (z read through one,
    out / dout through the other); dps: DM_FLAG_DOUT_PER_SEQ; ash: DM_FLAG_A_SHARED; acc: the accumulating three-direction forward."""
    return Case(fam, dtype, L, Dm, N, ndir, bpd, mode, z, tables, dps, ash, bcf32, groups, acc, ckpt, seed)


def _softplus(x):
    from oracle.mamba_ref import softplus_ref

    return softplus_ref(x)


def _silu(z):
    return z * torch.sigmoid(z)


# =====================================================================================================================================
# inputs: the long-memory construction of tests/test_kernels_gpu.py (_inputs_long_memory: A and dt as the model initialises them, dt arriving
# as delta + bias before the softplus) with every launch holding slow, middle, fast and "ends" channels (d % 4), after HEAD in test_ssd_gpu.py
# =====================================================================================================================================
@functools.lru_cache(maxsize=None)
def inputs(c):
    """Host tensors of a case in the I/O dtype (A, D, bias fp32) and the row tables.  Channel d is slow (A = -0.01 (n + 1), dt ~ 1e-3),
    middle (A = -0.3 (n + 1), dt ~ 0.02), fast (A = -16 - n / 8, dt ~ 0.1) or 'ends' (A = -(n + 1); pre-activation -12 + 0.3 randn: the
    series branch of softplus_f; every 40th token +25: the identity branch, a reset) by d % 4.  dt = level exp(0.3 randn)."""
    S, L, Dm, N, dt_ = c.ndir * c.bpd, c.L, c.Dm, c.N, c.dtype
    g = torch.Generator().manual_seed(7919 * c.seed + 31 * L + Dm + N + (1 if dt_ == F16 else 0))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    reg = torch.arange(Dm) % 4
    n1 = torch.arange(N, dtype=torch.float64)[None] + 1.0
    A = torch.where(reg[:, None] == 0, -0.01 * n1, torch.where(reg[:, None] == 1, -0.3 * n1, torch.where(reg[:, None] == 2, -16.0 - (n1 - 1) / 8, -n1)))
    A = A * torch.exp(0.2 * rn(Dm))[:, None]
    if c.ash:
        A = A[:, :1].expand(Dm, N).contiguous()
    level = torch.tensor([1e-3, 0.02, 0.1, 1.0], dtype=torch.float64)[reg]
    pre = torch.log(torch.expm1(level * torch.exp(0.3 * rn(S, L, Dm))))
    spike = ((torch.arange(L)[None] + 7 * torch.arange(S)[:, None]) % 40 == 5)[:, :, None]
    pre = torch.where(reg == 3, torch.where(spike, torch.full_like(pre, 25.0), -12.0 + 0.3 * rn(S, L, Dm)), pre)
    bias = torch.where(reg == 3, torch.full_like(level, -12.0), torch.log(torch.expm1(level))).float()
    if c.mode == 1:
        delta = (pre - bias.double()).to(dt_)
    else:                                                   # modes 0 and 2 take a positive step as it is
        bias = (0.1 * torch.where(reg == 3, torch.full_like(level, math.exp(-12.0)), level)).float() if c.mode == 0 else None
        delta = (_softplus(pre) - (bias.double() if c.mode == 0 else 0.0)).clamp_min(0.0).to(dt_)
    nz = c.bpd if c.tables else S
    G = c.groups
    t = dict(u=rn(S, L, Dm).to(dt_), delta=delta, z=rn(nz, L, Dm).to(dt_) if c.z else None, A=A.float(), bias=bias, D=rn(Dm).float(),
             B=rn(S, L, G * N).to(dt_), C=rn(S, L, G * N).to(dt_),
             dout=rn(S if (c.dps or not c.tables) else c.bpd, L, Dm).to(dt_))
    perm = lambda: torch.stack([torch.randperm(L, generator=g) for _ in range(c.ndir)])
    t["zperm"], t["operm"] = (perm(), perm()) if c.tables else (None, None)
    return t


def gather(c, defect=None):
    """fp64 operands in SCAN order [S, L, ..]: what step l of sequence s = k bpd + b reads through its tables."""
    t = inputs(c)
    S, L = c.ndir * c.bpd, c.L
    d = lambda v: v.double()
    q = dict(u=d(t["u"]), raw=d(t["delta"]), A=d(t["A"]), D=d(t["D"]), bias=None if t["bias"] is None else d(t["bias"]),
             B=d(t["B"]).view(S, L, c.groups, c.N), C=d(t["C"]).view(S, L, c.groups, c.N))
    q["gidx"] = torch.arange(c.Dm) // (c.Dm // c.groups)
    if c.tables:
        zs, gs = [], []
        for s in range(S):
            k, b = divmod(s, c.bpd)
            zi = t["operm"][k] if defect == "z_through_out_table" else t["zperm"][k]
            if c.z:
                zs.append(d(t["z"][b])[zi])
            gs.append(d(t["dout"][s if c.dps else b])[t["operm"][k]])
        q["z"], q["g"] = (torch.stack(zs) if c.z else None), torch.stack(gs)
    else:
        q["z"], q["g"] = (d(t["z"]) if c.z else None), d(t["dout"])
    return q


def _activation(c, q):
    """dt, softplus' and the pre-activation x, [S, L, Dm]."""
    if c.mode == 2:
        dt = q["raw"]
        # (past 20 the oracle's softplus is the identity, its derivative 1: 1 - e^-dt differs from that by < 2^-24 / 8, inside sp')
        return dt, torch.where(dt > 20.0, torch.ones_like(dt), -torch.expm1(-dt)), torch.where(dt > 20.0, dt, torch.log(torch.expm1(dt.clamp(min=1e-300, max=20.0))))
    x = q["raw"] + (q["bias"] if q["bias"] is not None else 0.0)
    if c.mode == 0:
        return x, torch.ones_like(x), x
    return _softplus(x), torch.where(x > 20.0, torch.ones_like(x), torch.sigmoid(x)), x


def scatter(c, v, which):
    """Scan-order rows [S, L, Dm] -> the kernel's rows: through out_row_index ('o') or z_row_index ('z') of the sequence's direction."""
    if not c.tables:
        return v
    t = inputs(c)
    out = torch.empty_like(v)
    for s in range(v.shape[0]):
        out[s] = out[s].index_copy(0, t["operm" if which == "o" else "zperm"][s // c.bpd], v[s])
    return out


def mfma_red(c):
    """B2: the instantiations that round the dB / dC products to bf16."""
    return c.dtype == BF16 and (c.fam == "K2c" or c.N <= 32)


# =====================================================================================================================================
# the closed form: reference (round=False), emulation (round=True), defects
# =====================================================================================================================================
DEFECTS = {
    # name: (outputs that must catch it, predicate on the case)
    "slot0_zero": (("dC", "dz"), lambda c: c.L % 4 == 0 and c.fam in ("K2", "K2c")),
    "carry_dropped": (("du", "ddelta", "dB", "dA"), lambda c: c.L > 8 and c.fam in ("K2", "K2c")),
    "fold_without_Q": (("du", "ddelta", "dB", "dA"), lambda c: c.fam == "K2c"),
    "decay_off_by_one": (("du", "ddelta", "dB", "dA"), lambda c: c.L >= 5 and c.fam == "K2" and c.N == 16 and not c.ash),
    "ddelta_without_dlA": (("ddelta", "dbias"), lambda c: c.L >= 5 and c.fam in ("K2", "K2c")),
    "mode2_without_softplus_grad": (("ddelta", "dbias"), lambda c: c.mode == 2),
    "dz_without_Du": (("dz",), lambda c: c.z and c.fam in ("K2", "K2c")),
    "z_through_out_table": (("out", "dz", "du"), lambda c: c.z and c.tables and c.L >= 5),
    "tail_dout_not_zeroed": (("du", "ddelta", "dA", "dD"), lambda c: c.L % 4 != 0 and c.fam in ("K2", "K2c")),
    "pad_lanes_in_dBC": (("dB", "dC"), lambda c: c.Dm % 64 != 0 and c.fam in ("K2", "K2c")),
    "lane_group_missing": (("dB", "dC"), lambda c: c.fam in ("K2", "K2c")),
    "ckpt_pair_swapped": (("dC", "dz", "ddelta", "dA"), lambda c: c.L >= 5 and c.fam in ("K2", "K2c")),
    "partial_row_dropped": (("dB", "dC"), lambda c: c.Dm > 256 and c.fam == "K2"),
    "acc_stores": (("out",), lambda c: c.acc),
}


def manual(c, round=False, defect=None):
    """{output: fp64 tensor in the kernel's layout}.  round: the I/O rounding applied where the kernels round (module docstring), all other
    arithmetic fp64.  defect: one of DEFECTS, applied to the otherwise exact form."""
    q = gather(c, defect)
    S, L, Dm, N = c.ndir * c.bpd, c.L, c.Dm, c.N
    idt = lambda v: v
    rio = (lambda v: v.to(c.dtype).double()) if round else idt
    rck = (lambda v: v.to(BF16).double()) if (round and c.dtype == BF16) else idt
    rpr = (lambda v: v.to(BF16).double()) if (round and mfma_red(c)) else idt
    u, A, D, z, g = q["u"], q["A"], q["D"], q["z"], q["g"]
    dt, spf, _ = _activation(c, q)
    if defect == "mode2_without_softplus_grad":
        spf = torch.ones_like(spf)
    sil = _silu(z) if c.z else torch.ones_like(u)
    sg = torch.sigmoid(z) if c.z else None
    dsil = sg * (1 + z * (1 - sg)) if c.z else None
    row = lambda l: min(l, L - 1)                                    # rows past the end re-read row L - 1

    def step(l):
        l = row(l)
        Bl, Cl = q["B"][:, l][:, q["gidx"]], q["C"][:, l][:, q["gidx"]]                  # [S, Dm, N]
        a = torch.exp(dt[:, l, :, None] * A)
        return a, (dt[:, l] * u[:, l])[..., None] * Bl, Bl, Cl

    Lp = -(-L // SUB) * SUB
    hs = [torch.zeros(S, Dm, N, dtype=torch.float64)]
    ypre = torch.empty(S, L, Dm, dtype=torch.float64)
    for l in range(Lp if defect == "tail_dout_not_zeroed" else L):
        a, b, _, Cl = step(l)
        hs.append(a * hs[-1] + b)
        if l < L:
            ypre[:, l] = (hs[-1] * Cl).sum(-1) + D * u[:, l]
    y = ypre * sil
    res = {}
    if c.acc:                                                       # F2: one token-order buffer, a rounding per direction
        t = inputs(c)
        acc = torch.zeros(c.bpd, L, Dm, dtype=torch.float64)
        for k in range(c.ndir):
            yk = torch.zeros_like(acc).index_copy(1, t["operm"][k], y[k * c.bpd:(k + 1) * c.bpd])
            acc = rio(yk if (k == 0 or defect == "acc_stores") else acc + yk)
        res["out"] = acc
    else:
        res["out"], res["out_pre"] = rio(scatter(c, y, "o")), scatter(c, y, "o")
    res["last_state"] = hs[L].transpose(1, 2)                                   # [S, N, Dm] fp32
    K = list(range(SUB, L, SUB))
    res["ckpt"] = torch.stack([rck(hs[L])] + [rck(hs[k]) for k in K], 1).transpose(2, 3)          # [S, slots, N, Dm]; slot 0 = end state
    if c.fam in ("K1", "K1c"):
        return res

    # B1: the states the sweep sees
    hb = list(hs)
    if round or defect in ("slot0_zero", "ckpt_pair_swapped"):
        for k in range(1, L + 1):
            if k % SUB == 0:
                hb[k] = rck(hs[k])
                if defect == "ckpt_pair_swapped":
                    hb[k] = hb[k].view(S, Dm, N // 2, 2).flip(-1).reshape(S, Dm, N)
                if defect == "slot0_zero" and k == L:
                    hb[k] = torch.zeros_like(hb[k])
            else:
                a, b, _, _ = step(k - 1)
                hb[k] = a * hb[k - 1] + b
    LC = {"K2": 8, "K2c": 8 if L <= 56 else 28}[c.fam]              # staging chunk (K2), wave chunk (K2c)
    folded = None
    if defect == "fold_without_Q":                                  # the carry entering chunk j = the plain sum of the local carries to its right
        loc, carry = {}, torch.zeros(S, Dm, N, dtype=torch.float64)
        for k in range(L, 0, -1):
            a, _, _, Cl = step(k - 1)
            carry = a * (Cl * (g[:, k - 1] * sil[:, k - 1])[..., None] + (0.0 if (k % LC == 0 or k == L) else carry))
            if (k - 1) % LC == 0:
                loc[k - 1] = carry
        folded = {k: sum(v for kk, v in loc.items() if kk >= k) for k in loc}
    out = {n: torch.zeros(S, L, Dm, dtype=torch.float64) for n in ("du", "ddelta", "dz")}
    dB, dC = torch.zeros(S, L, N, dtype=torch.float64), torch.zeros(S, L, N, dtype=torch.float64)
    dA, dD, dbias = torch.zeros(S, Dm, N, dtype=torch.float64), torch.zeros(S, Dm, dtype=torch.float64), torch.zeros(S, Dm, dtype=torch.float64)
    chan = torch.ones(Dm, dtype=torch.float64)                      # weight of a channel in the dB / dC sums
    if defect == "pad_lanes_in_dBC":
        gc = 64 if c.fam == "K2c" else 256
        chan[-1] += -(-Dm // gc) * gc - Dm
    if defect == "lane_group_missing":
        chan[(torch.arange(Dm) % 64) // 16 == 3] = 0.0
    if defect == "partial_row_dropped":
        chan[256:] = 0.0
    carry = torch.zeros(S, Dm, N, dtype=torch.float64)
    for k in range(Lp if defect == "tail_dout_not_zeroed" else L, 0, -1):
        l = row(k - 1)
        a, _, Bl, Cl = step(k - 1)
        if defect == "decay_off_by_one" and k < L and k % SUB != 0:
            a = step(k)[0]
        if k < L and k % LC == 0:
            if defect == "carry_dropped":
                carry = torch.zeros_like(carry)
            if defect == "fold_without_Q":
                carry = folded[k]
        gy = g[:, l] * sil[:, l]
        lam = Cl * gy[..., None] + carry
        carry = a * lam
        Gt = carry * hb[k - 1]
        dA += Gt * dt[:, l, :, None]
        GB = (lam * Bl).sum(-1)
        dlA = (A * Gt).sum(-1)
        ddl = (u[:, l] * GB + (0.0 if defect == "ddelta_without_dlA" else dlA)) * spf[:, l]
        dD += gy * u[:, l]
        dbias += ddl
        if k > L:
            continue                                                # a tail step stores nothing
        dC[:, l] = (rpr(hb[k] * gy[..., None]) * chan[None, :, None]).sum(1)
        dB[:, l] = (rpr(lam * (dt[:, l] * u[:, l])[..., None]) * chan[None, :, None]).sum(1)
        out["ddelta"][:, l] = ddl
        out["du"][:, l] = dt[:, l] * GB + gy * D
        if c.z:
            yb = (hb[k] * Cl).sum(-1) + (0.0 if defect == "dz_without_Du" else D * u[:, l])
            out["dz"][:, l] = g[:, l] * yb * dsil[:, l]
    res.update(du=rio(out["du"]), ddelta=rio(out["ddelta"]), dB=dB, dC=dC, dA=dA.sum(0), dD=dD.sum(0), du_pre=out["du"], ddelta_pre=out["ddelta"])
    if c.z:
        res["dz"], res["dz_pre"] = rio(scatter(c, out["dz"], "z")), scatter(c, out["dz"], "z")
    if c.mode != 0 or q["bias"] is not None:
        res["dbias"] = dbias.sum(0)
    return res


# =====================================================================================================================================
# the bounds
# =====================================================================================================================================
def _perr(ax, ex, ay, ey):
    """Error of a product of two quantities known to (|x|, ex), (|y|, ey)."""
    return ax * ey + ay * ex + ex * ey


def bounds(c):
    """{output: per-element bound} in the layout of `manual` (module docstring: BOUNDS)."""
    q = gather(c)
    S, L, Dm, N = c.ndir * c.bpd, c.L, c.Dm, c.N
    e, uu, T = EPS32, UNIT[c.dtype], TINY[c.dtype]
    DK = 31.0 if c.fam in ("K1c", "K2c") else 3.0
    u, A, D, z, g = q["u"], q["A"], q["D"], q["z"], q["g"]
    dt, spf, x = _activation(c, q)
    if c.mode == 2:
        ddt = torch.zeros_like(dt)
    elif c.mode == 0:
        ddt = e * x.abs()
    else:
        s_, E = torch.sigmoid(x), torch.exp(x.clamp(max=21.0))
        ddt = torch.where(x > 20.0, e * x.abs(), torch.where(E < 2.0 ** -12, dt * e * (3 * x.abs() + 7), e * (s_ * (3 * x.abs() + 2) + 1 + 4 * dt)))
    aA = A.abs()
    if c.z:
        sg = torch.sigmoid(z)
        sil, CG = z * sg, 7 + 2 * z.abs()
        f = 1 + z * (1 - sg)
        ferr = e * (z.abs() * (6 + 2 * z.abs()) + 2)
    else:
        sil, CG = torch.ones_like(u), torch.zeros_like(u)
    st = lambda v, err: uu * (v.abs() + err) + T + err              # a stored 16-bit (or fp32) value

    def step(l):
        Bl, Cl = q["B"][:, l][:, q["gidx"]], q["C"][:, l][:, q["gidx"]]
        return torch.exp(dt[:, l, :, None] * A), Bl, Cl

    # forward: h, habs, F (K1 / K1c's own state error), E (the sweep's)
    zero = torch.zeros(S, Dm, N, dtype=torch.float64)
    h, habs, F, ck = [zero], [zero], [zero], [zero]
    b = {}
    yerr = torch.empty(S, L, Dm, dtype=torch.float64)
    ypre = torch.empty(S, L, Dm, dtype=torch.float64)
    yS = torch.empty(S, L, Dm, dtype=torch.float64)
    for l in range(L):
        a, Bl, Cl = step(l)
        bk = (dt[:, l] * u[:, l])[..., None] * Bl
        adt = aA * dt[:, l, :, None]
        loc = e * (a * habs[-1] * (DK * adt + 4) + 4 * bk.abs()) + ddt[:, l, :, None] * (aA * a * habs[-1] + (Bl * u[:, l, :, None]).abs()) \
            + TINY32 * (1 + habs[-1])
        F.append(a * F[-1] + loc)
        h.append(a * h[-1] + bk)
        habs.append(a * habs[-1] + bk.abs())
        k = l + 1
        ck.append(uu * (h[k].abs() + F[k]) + T if (c.dtype == BF16 and k % SUB == 0) else a * ck[-1])
        ypre[:, l] = (h[k] * Cl).sum(-1) + D * u[:, l]
        yS[:, l] = (h[k] * Cl).abs().sum(-1) + (D * u[:, l]).abs()
        yerr[:, l] = (Cl.abs() * F[k]).sum(-1) + (N + 2) * e * yS[:, l]
    oerr = yerr * sil.abs() + (ypre * sil).abs() * (CG + 1) * e                 # before the store
    y = ypre * sil
    res = {}
    if c.acc:
        t = inputs(c)
        acc, aerr = torch.zeros(c.bpd, L, Dm, dtype=torch.float64), torch.zeros(c.bpd, L, Dm, dtype=torch.float64)
        for k in range(c.ndir):
            sl = slice(k * c.bpd, (k + 1) * c.bpd)
            acc = acc + torch.zeros_like(acc).index_copy(1, t["operm"][k], y[sl])
            aerr = aerr + torch.zeros_like(acc).index_copy(1, t["operm"][k], oerr[sl]) + (e * acc.abs() if k else 0.0)
            aerr = st(acc, aerr)
        res["out"] = aerr
    else:
        res["out"] = scatter(c, st(y, oerr), "o")
    res["out_pre"] = scatter(c, oerr, "o") if not c.acc else None
    K = list(range(SUB, L, SUB))
    ckb = lambda k: (uu * (h[k].abs() + F[k]) + T + F[k]) if c.dtype == BF16 else F[k]
    res["ckpt"] = torch.stack([ckb(L)] + [ckb(k) for k in K], 1).transpose(2, 3)
    res["last_state"] = F[L].transpose(1, 2)
    if c.fam in ("K1", "K1c"):
        return res

    Eh = [F[k] + ck[k] for k in range(L + 1)]
    fin = {n: torch.zeros(S, L, Dm, dtype=torch.float64) for n in ("du", "ddelta", "dz")}
    pre = {n: torch.zeros(S, L, Dm, dtype=torch.float64) for n in ("du", "ddelta", "dz")}
    dB, dC = torch.zeros(S, L, N, dtype=torch.float64), torch.zeros(S, L, N, dtype=torch.float64)
    dAe, dAs = torch.zeros(S, Dm, N, dtype=torch.float64), torch.zeros(S, Dm, N, dtype=torch.float64)
    dDe, dDs, dbe, dbs = (torch.zeros(S, Dm, dtype=torch.float64) for _ in range(4))
    carry, cabs, cerr = zero, zero, zero
    ub, Tb = (UNIT[BF16], TINY[BF16]) if mfma_red(c) else (0.0, 0.0)
    for k in range(L, 0, -1):
        l = k - 1
        a, Bl, Cl = step(l)
        adt = aA * dt[:, l, :, None]
        gy = g[:, l] * sil[:, l]
        gye = gy.abs() * CG[:, l] * e
        Cgy = (Cl * gy[..., None]).abs()
        lam = Cl * gy[..., None] + carry
        labs = Cgy + cabs
        lerr = Cgy * (CG[:, l, :, None] + 1) * e + e * labs + cerr
        arel = e * (3 + DK * adt) + aA * ddt[:, l, :, None]
        carry, cabs, cerr = a * lam, a * labs, a * lerr + a * labs * arel
        hp, hk = h[k - 1], h[k]
        Gt = carry * hp
        Gte = _perr(carry.abs(), cerr, hp.abs(), Eh[k - 1]) + e * Gt.abs()
        dtl, ul = dt[:, l], u[:, l]
        dAe += _perr(Gt.abs(), Gte, dtl[..., None], ddt[:, l, :, None]) + e * (Gt * dtl[..., None]).abs()
        dAs += (Gt * dtl[..., None]).abs()
        GB, GBs = (lam * Bl).sum(-1), (labs * Bl.abs()).sum(-1)
        GBe = (lerr * Bl.abs()).sum(-1) + (N + 2) * e * GBs
        dlA, dlAs = (A * Gt).sum(-1), (aA * Gt.abs()).sum(-1)
        dlAe = (aA * Gte).sum(-1) + (N + 5) * e * dlAs
        ddp = ul * GB + dlA
        ddpe = ul.abs() * GBe + dlAe + 2 * e * ((ul * GB).abs() + dlA.abs())
        spe = torch.zeros_like(dtl) if c.mode == 0 else e * (2 + 2 * dtl + spf[:, l]) + ddt[:, l]
        ddl = ddp * spf[:, l]
        ddle = _perr(ddp.abs(), ddpe, spf[:, l], spe) + e * ddl.abs()
        pre["ddelta"][:, l], fin["ddelta"][:, l] = ddle, st(ddl, ddle)
        dbe += ddle
        dbs += ddl.abs()
        duv = dtl * GB + gy * D
        due = _perr(GB.abs(), GBe, dtl, ddt[:, l]) + (gye + e * gy.abs()) * D.abs() + 2 * e * ((dtl * GB).abs() + (gy * D).abs())
        pre["du"][:, l], fin["du"][:, l] = due, st(duv, due)
        dDe += (gye + e * gy.abs()) * ul.abs()
        dDs += (gy * ul).abs()
        if c.z:
            yb = (hk * Cl).sum(-1) + D * ul
            ybe = (Cl.abs() * Eh[k]).sum(-1) + (N + 2) * e * yS[:, l]
            gsz = g[:, l] * sg[:, l]
            dzv = gsz * yb * f[:, l]
            dze = (gsz * f[:, l]).abs() * ybe + (gsz * yb).abs() * ferr[:, l] + (gsz.abs() * ybe) * ferr[:, l] + dzv.abs() * (CG[:, l] + 4) * e
            pre["dz"][:, l], fin["dz"][:, l] = dze, st(dzv, dze)
        pC = hk * gy[..., None]
        pCe = _perr(hk.abs(), Eh[k], gy.abs()[..., None], gye[..., None]) + e * pC.abs()
        pB = lam * (dtl * ul)[..., None]
        dtu_e = (ddt[:, l] * ul.abs() + e * (dtl * ul).abs())[..., None]
        pBe = _perr(lam.abs(), lerr, (dtl * ul).abs()[..., None], dtu_e) + e * pB.abs()
        dC[:, l] = (pCe + ub * (pC.abs() + pCe) + Tb).sum(1) + Dm * e * pC.abs().sum(1)
        dB[:, l] = (pBe + ub * (pB.abs() + pBe) + Tb).sum(1) + Dm * e * pB.abs().sum(1)
    n_acc = (L + S + 2) * e
    res.update(du=fin["du"], ddelta=fin["ddelta"], dB=dB, dC=dC, dA=(dAe + n_acc * dAs).sum(0), dD=(dDe + n_acc * dDs).sum(0),
               du_pre=pre["du"], ddelta_pre=pre["ddelta"])
    if c.z:
        res["dz"], res["dz_pre"] = scatter(c, fin["dz"], "z"), scatter(c, pre["dz"], "z")
    if c.mode != 0 or q["bias"] is not None:
        res["dbias"] = (dbe + n_acc * dbs).sum(0)
    return res


@functools.lru_cache(maxsize=None)
def analysis(c):
    """(reference, bound) of a case, computed once and left unchanged."""
    return manual(c), bounds(c)


OUTPUTS = ("out", "ckpt", "last_state", "du", "ddelta", "dz", "dB", "dC", "dA", "dD", "dbias")


def _ratio(got, ref, tol):
    d = (got.double() - ref).abs()
    r = (d / tol).nan_to_num(nan=1e30, posinf=1e30)
    return torch.where(d == 0, torch.zeros_like(r), r)                # a bound of 0 (dA at L = 1: no state before step 0) asks for the exact value


def check(c, name, got, what=None):
    """got against the reference within the bound, every element; records the worst ratio."""
    ref, tol = analysis(c)
    r = _ratio(got, ref[name], tol[name])
    worst = float(r.max())
    key = (what or c.fam, name, NAME[c.dtype], c.N)
    WORST[key] = max(WORST.get(key, 0.0), worst)
    assert got.shape == ref[name].shape
    i = int(r.reshape(-1).argmax())
    assert worst <= 1.0, f"{c}: {name} worst |got - ref| / bound {worst:.3f} at flat index {i} (ref {float(ref[name].reshape(-1)[i]):.4e}, bound {float(tol[name].reshape(-1)[i]):.3e})"


def report():
    for k in sorted(WORST, key=str):
        print(f"worst |got - ref| / bound  {k[0]:10s} {k[1]:10s} {k[2]:4s} N={k[3]:3d}: {WORST[k]:.4f}")


# =====================================================================================================================================
# the cases of the device tests (tests/test_scan_bounds_gpu.py), also the cases of the sharpness and defect tests here
# =====================================================================================================================================
PATTERNS = {
    "gated": dict(),
    "no_z": dict(z=False),
    "mode0": dict(mode=0),
    "three_dirs": dict(ndir=3, bpd=2, tables=True),
    "dout_per_seq": dict(ndir=2, bpd=1, tables=True, dps=True),
    "mamba2": dict(ndir=2, bpd=2, tables=True, dps=True, ash=True),
    "hoisted": dict(ndir=3, bpd=1, tables=True, mode=2, z=False),
    "bc_fp32": dict(bcf32=True, ndir=1, bpd=2),
}


def bwd_cases(dtype):
    """K2 and K2c at d_state 16 (section 5 of the issue): every L of a family plain, every call pattern at two lengths, the model's at 196."""
    cs = []
    for L in (1, 4, 5, 8, 11, 29):
        cs.append(case("K2", dtype, L, 72, ndir=1, bpd=2, seed=1))
    for L in (11, 29):
        cs.append(case("K2", dtype, L, 320, seed=2))
        cs += [case("K2", dtype, L, 72, seed=3, **kw) for n, kw in PATTERNS.items() if n != "gated"]
    cs.append(case("K2", dtype, 196, 72, seed=4, **PATTERNS["three_dirs"]))
    cs.append(case("K2", dtype, 196, 72, seed=4, **PATTERNS["hoisted"]))
    for L in (17, 20, 56, 57, 60, 183):
        cs.append(case("K2c", dtype, L, 72, ndir=1, bpd=2, seed=5))
    for L in (20, 60):
        cs += [case("K2c", dtype, L, 72, seed=6, **kw) for n, kw in PATTERNS.items() if n != "gated"]
    cs.append(case("K2c", dtype, 196, 72, seed=7, **PATTERNS["three_dirs"]))
    cs.append(case("K2c", dtype, 196, 72, seed=7, **PATTERNS["hoisted"]))
    return cs


def bwd_cases_wide(dtype):
    """K2 at the other widths (the build has them unless DM_FAST_BUILD): plain and with tables; the one-exp form at 64 and 128."""
    cs = []
    for N, Dm in ((8, 200), (32, 200), (64, 96), (128, 96)):
        for L in (11, 29):
            cs.append(case("K2", dtype, L, Dm, N=N, seed=8))
            cs.append(case("K2", dtype, L, Dm, N=N, seed=9, **PATTERNS["three_dirs"]))
    for N in (64, 128):
        cs.append(case("K2", dtype, 29, 96, N=N, seed=10, **PATTERNS["mamba2"]))
    return cs


def fwd_cases(dtype):
    cs = []
    for L in (1, 7, 8, 9, 17):
        cs.append(case("K1", dtype, L, 72, ndir=1, bpd=2, seed=11))
        cs.append(case("K1", dtype, L, 200, seed=12, **PATTERNS["three_dirs"]))
    cs.append(case("K1", dtype, 196, 72, seed=13, **PATTERNS["three_dirs"]))
    cs.append(case("K1", dtype, 196, 200, seed=13, ckpt=False))
    cs.append(case("K1", dtype, 17, 72, seed=14, ckpt=False, **PATTERNS["hoisted"]))
    for L in (17, 196):
        cs.append(case("K1", dtype, L, 72, seed=15, ndir=3, bpd=2, tables=True, acc=True))
    for N in (8, 32, 64, 128):
        cs.append(case("K1", dtype, 17, 72, N=N, seed=16, ndir=2, bpd=1, tables=True))
    cs.append(case("K1", dtype, 17, 72, N=64, seed=17, **PATTERNS["mamba2"]))
    for L in (57, 100, 183, 196):
        cs.append(case("K1c", dtype, L, 72, seed=18, **PATTERNS["three_dirs"]))
        cs.append(case("K1c", dtype, L, 72, seed=19, ndir=1, bpd=2, ckpt=False))
    for fam, L in (("K1", 17), ("K1c", 60)):
        for Dm in (128, 256):
            cs.append(case(fam, dtype, L, Dm, seed=20, groups=2, ckpt=False, ndir=1, bpd=2))
    return cs


def all_cases(dtype):
    return bwd_cases(dtype) + bwd_cases_wide(dtype) + fwd_cases(dtype)


def cid(c):
    on = [n for n in ("tables", "dps", "ash", "bcf32", "acc") if getattr(c, n)]
    return f"{c.fam}-{NAME[c.dtype]}-L{c.L}-D{c.Dm}-N{c.N}-{c.ndir}x{c.bpd}-m{c.mode}{'z' if c.z else ''}-g{c.groups}-{'ck' if c.ckpt else 'nock'}" + "".join("-" + n for n in on)


# =====================================================================================================================================
# CPU tests
# =====================================================================================================================================
def _autograd(c):
    """Forward by selective_scan_ref and every gradient by fp64 autograd through it, in the layout of `manual`."""
    from oracle.mamba_ref import selective_scan_ref

    q = gather(c)
    S = c.ndir * c.bpd
    leaf = lambda v: v.clone().requires_grad_(True)
    u, A, D, B, C = leaf(q["u"]), leaf(q["A"]), leaf(q["D"]), leaf(q["B"]), leaf(q["C"])
    z = leaf(q["z"]) if c.z else None
    _, _, x = _activation(c, q)
    if c.mode == 2:
        raw, bias = leaf(x), leaf(torch.zeros(c.Dm, dtype=torch.float64))
    else:
        raw, bias = leaf(q["raw"]), (leaf(q["bias"]) if q["bias"] is not None else None)
    cm = lambda v: v.permute(0, 2, 1)
    y, last = selective_scan_ref(cm(u), cm(raw), A, B.permute(0, 2, 3, 1), C.permute(0, 2, 3, 1), D, z=None if z is None else cm(z), delta_bias=bias,
                                 delta_softplus=c.mode != 0, return_last_state=True)
    y = cm(y)
    (y * q["g"]).sum().backward()
    res = dict(out=scatter(c, y.detach(), "o"), last_state=last.detach().transpose(1, 2), du=u.grad, ddelta=raw.grad, dB=B.grad[:, :, 0], dC=C.grad[:, :, 0],
               dA=A.grad, dD=D.grad)
    if c.z:
        res["dz"] = scatter(c, z.grad, "z")
    if bias is not None:
        res["dbias"] = bias.grad
    return res


PIN = [case("K2", F16, 13, 24, ndir=1, bpd=2, seed=21)] + [case("K2", BF16, 13, 24, seed=22, **kw) for kw in PATTERNS.values()] \
    + [case("K2", BF16, 13, 24, N=8, seed=23, ndir=2, bpd=2, tables=True, mode=0, z=False)]


@pytest.mark.parametrize("c", PIN, ids=cid)
def test_manual_equals_autograd(c):
    """The closed form restates the oracle: forward, last state and every gradient at 1e-12 max|ref| per output, for every call pattern
    (delta modes 0 / 1 / 2, with and without z, row tables, batch_per_dir, DOUT_PER_SEQ, A_SHARED, fp32 B / C)."""
    want, got = _autograd(c), manual(c)
    assert set(want) <= set(got)
    for k, w in want.items():
        assert float((got[k] - w).abs().max()) <= 1e-12 * float(w.abs().max()), k


def test_manual_forward_with_groups_equals_the_oracle():
    """ngroups = 2 (forward only): channels of group 1 read B / C columns N .. 2N; the accumulating form equals the per-direction sum."""
    from oracle.mamba_ref import selective_scan_ref

    c = case("K1", F16, 9, 128, groups=2, ckpt=False, ndir=1, bpd=2, seed=24)
    q = gather(c)
    cm = lambda v: v.permute(0, 2, 1)
    y = selective_scan_ref(cm(q["u"]), cm(q["raw"]), q["A"], q["B"].permute(0, 2, 3, 1), q["C"].permute(0, 2, 3, 1), q["D"], z=cm(q["z"]),
                           delta_bias=q["bias"], delta_softplus=True)
    assert float((manual(c)["out"] - cm(y)).abs().max()) <= 1e-12 * float(y.abs().max())
    assert not torch.equal(q["B"][:, :, 0], q["B"][:, :, 1])
    ca = case("K1", F16, 9, 24, ndir=3, bpd=2, tables=True, acc=True, seed=25)
    y, t = manual(ca._replace(acc=False))["out"], inputs(ca)
    assert float((manual(ca)["out"] - y.view(3, 2, 9, 24).sum(0)).abs().max()) <= 1e-12 * float(y.abs().max())


MARGIN = [case("K2", dt, L, 72, seed=26, **kw) for dt in (BF16, F16, F32) for L, kw in ((29, PATTERNS["three_dirs"]), (11, PATTERNS["hoisted"]),
                                                                                         (196, PATTERNS["gated"]))] \
    + [case("K1", dt, 17, 72, seed=27, ndir=3, bpd=2, tables=True, acc=True) for dt in (BF16, F16)] + [case("K2c", BF16, 60, 72, seed=28), case("K2", BF16, 29, 96, N=64, seed=28)]


@pytest.mark.parametrize("c", MARGIN, ids=cid)
def test_emulation_stays_inside_the_bound(c):
    """The fp64 emulation with the kernels' rounding places: <= 0.5 of the bound for the fp32 outputs (dA, dD, dbias, last_state, fp32
    checkpoints, fp32 dB / dC) and for stored values before their last rounding; <= 1 where one rounding charged in full is the whole error."""
    ref, tol = analysis(c)
    emu = manual(c, round=True)
    for k in emu:
        if k.endswith("_pre"):
            continue
        r = float(_ratio(emu[k], ref[k], tol[k]).max())
        WORST[("emulation", k, NAME[c.dtype], c.N)] = max(WORST.get(("emulation", k, NAME[c.dtype], c.N), 0.0), r)
        # one rounding charged in full is the whole error: the stored 16-bit outputs; with bf16 I/O the checkpoints, what the sweep makes
        # of them (dC = h gy; dA and dbias through Gt = carry h: a slow channel's state keeps its rounding error from slot to slot, so the
        # errors of the steps add up with one sign) and the bf16 products of dB / dC
        one_rounding = k in ("out", "du", "ddelta", "dz") or (c.dtype == BF16 and k in ("ckpt", "dA", "dbias", "dB", "dC"))
        assert r <= (1.0 if one_rounding else 0.5), (k, r)
    for k in ("out_pre", "du_pre", "ddelta_pre", "dz_pre"):          # the values before their last rounding (bf16: checkpoints charged in full)
        if k in emu and tol.get(k) is not None:
            r = float(_ratio(emu[k], ref[k], tol[k]).max())
            assert r <= (1.0 if c.dtype == BF16 else 0.5), (k, r)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_bounds_are_sharp(dtype):
    """A condition, not a measurement: on every device case the median over ALL elements of bound / |ref| is <= 1 for every output, so
    a kernel cannot replace most of an output by zero and pass.  Prints the medians."""
    worst = {}
    for c in all_cases(dtype):
        ref, tol = analysis(c)
        for k in OUTPUTS:
            if k in ref and tol.get(k) is not None:
                m = float((tol[k] / ref[k].abs().clamp_min(1e-300)).median())
                worst[(c.fam, k)] = max(worst.get((c.fam, k), 0.0), m)
                assert m <= 1.0, (cid(c), k, m)
                assert bool(torch.isfinite(tol[k]).all()) and bool((tol[k] >= 0).all()), (cid(c), k)
    for k in sorted(worst):
        print(f"largest median bound / |ref|  {k[0]:4s} {k[1]:10s} {NAME[dtype]}: {worst[k]:.3e}")


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_defects_exceed_the_bound(defect, dtype):
    """Each defect, applied inside `manual` to the fp64 reference, exceeds 4 x the bound on every output named for it, on at least one
    of the device cases named for it, at both 16-bit dtypes."""
    outs, pred = DEFECTS[defect]
    cs = [c for c in all_cases(dtype) if pred(c) and c.L <= 60 and c.N == 16][:6]
    assert cs, defect
    caught = {k: 0.0 for k in outs}
    for c in cs:
        ref, tol = analysis(c)
        bad = manual(c, defect=defect)
        for k in outs:
            if k in bad and k in ref:
                caught[k] = max(caught[k], float(_ratio(bad[k], ref[k], tol[k]).max()))
    print(defect, NAME[dtype], {k: f"{v:.1f}" for k, v in caught.items()})
    assert all(v > 4.0 for v in caught.values()), (defect, caught)


def test_scan_bwd_refuses_more_than_one_group():
    """dm_selective_scan_bwd and dm_selective_scan_bwd_n return DM_ERR_ARG before any launch for ngroups = 2, dim = 128 in an otherwise
    valid struct (K2 / K2c stage one B/C row and write one dB/dC partial row per workgroup), and dm_last_error names ngroups."""
    from diffma_amd import _lib

    lib = _lib.load()
    keep = (ctypes.c_float * 64)()
    p = ctypes.addressof(keep)
    for ng, want in ((2, -1), (0, -1)):
        a = _lib.dm_scan_bwd_args()
        a.nseq, a.seqlen, a.dim, a.dstate, a.ngroups = 1, 4, 128, 16, ng
        a.io_dtype, a.bc_dtype, a.ckpt_dtype, a.ckpt_every = 0, 0, 0, SUB
        for f in ("u", "delta", "dout", "A", "B", "C", "du", "ddelta", "dBC_partial", "dA_partial", "ckpt"):
            setattr(a, f, p)
        for f in ("u_sd", "dt_sd", "do_sd", "du_sd", "ddt_sd", "B_sn", "C_sn"):
            setattr(a, f, 1)
        assert int(lib.dm_selective_scan_bwd(ctypes.byref(a), None)) == want
        if ng == 2:
            msg = lib.dm_last_error().decode()
            assert "ngroups" in msg and "one B/C group" in msg, msg
            arr = (_lib.dm_scan_bwd_args * 2)(a, a)
            assert int(lib.dm_selective_scan_bwd_n(ctypes.cast(arr, ctypes.c_void_p), 2, None)) == want
            assert "ngroups" in lib.dm_last_error().decode()


def test_zz_error_to_bound_ratios():
    report()
