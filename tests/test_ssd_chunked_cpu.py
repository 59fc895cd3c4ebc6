"""dm_ssd_fwd_chunked (csrc/ssd_chunked.hip: the Mamba-2 SSD forward past one chunk, 1 <= L <= 1024): the parts that need no GPU.

Reference.  `_dual` of tests/test_ssd_gpu.py (fp64, chunk-free, pinned there to oracle.mamba2_ref.ssd_scan_ref).  `chunked` restates
the kernel header's decomposition in fp64 with the library's chunk length Q = dm_ssd_fwd_chunk_len(d_state):
    y_l    = [dual form over the keys of l's own chunk] + exp(s_l) sum_n C_l[n] h[n][p] + D x_l         (s: chunk-local prefix sums)
    h_next = exp(s_end) h + sum_{i in chunk} exp(s_end - s_i) dt_i B_i[n] x_i[p]
It equals `_dual` to 1e-12 (test), carries the defects, and with `rnd` given it is the emulation: fp64 arithmetic rounded exactly
where the kernel rounds.

Inputs.  The four head regimes, the two row tables per direction and the randn operands of tests/test_ssd_wide_cpu.inputs, restated
with the (directions, batch_per_dir) pair as an argument (that file looks it up in a table of its own lengths).  A second family,
"coherent", serves the state defects: B and C rows are one row common to the sequence plus 0.25 randn, x = |randn|, so that what a
state carries adds up instead of averaging out (with randn rows, overwriting the carry moves a d_state 128 bf16 output by 2 - 2.5
bounds only: the wide bf16 bound is about 0.2 of a randn output).  The common row is randn scaled by sqrt(4 / N) (C_l . B_i ~ 4), which
keeps |out| < 4096 in the fp64 reference (asserted), well inside fp16's range.

Bound.  u, T, EPS32, C32, K0f, P1, P2 as in tests/test_ssd_gpu.py's docstring and tests/test_ssd_wide_cpu.fwd_bound; chunk boundaries
are tile boundaries, so a pair (l, i) of ONE chunk sees the same alpha, gamma, delta whether the prefix sums are chunk-local or not
and is charged exactly as there (three roundings allowed, the kernel spends one: the score tile, sf_offdiag and sf_diag of ssd_fwd_common.h).
A pair whose key lies in an EARLIER chunk (nch = chunks between them >= 1) is charged what the kernel does on that path:
  * two 16-bit roundings: the weighted operand rnd(dt_i exp(s_end - s_i) x_ip) of the state update (`xw`) and the carried state
    rnd(h[n][p]) where the query tile reads it (`hb`; once however many chunks it crossed: h travels in fp32).  |h| is at most the
    S-form sum_i |B_in| w_i |x_ip| (1 + u), so both are relative to Wabs |x|:   ((1 + u)^2 - 1) Wabs
    and in the subnormal range absolute: T per weighted operand, which reaches the output through |C_l| . |B_i| and the decay from the
    end of the key's chunk (Mend), and T per state element, through exp(s_l - s_start) sum_n |C_ln| once per query:
        Ta[l] = T (1 + u) sum_i Gabs[l, i] Mend[l, i],      Tb[l] = T exp(s_l - s_start(l)) sum_n |C_ln|
  * fp32: the exponent of the pair's decay is now a sum of chunk-local prefix sums -- s_l local (EX), s_end of every chunk
    between (dec), s_end - s_i of the key's chunk (WT) -- each an 8-addition sum with the sign of A (10 EPS32 of its
    magnitude) and one more rounding for a difference; their magnitudes add up to at most 2 |s_l| + |s_i| (global), so
        C32x = C32 + 12 EPS32 |s_l|
    and the extra exp2s and products (one v_exp_f32 at 2 EPS32 and one product per link of the chain: 3 nch), the exp2 and the
    products of EX and WT, the chain's additions and the two extra accumulations (the state update over the chunk's keys, inside the
    2 (l + 1) already charged since l >= Q; the inter-chunk product over N states, inside 2 (N - 16) + 72):
        K0x = K0f + EPS32 (3 nch + 16)
    E[l, i] = ((1 + u)^2 - 1 + C32x + K0x) Wabs      for a key in an earlier chunk
    |out - ref| <= |silu z| (E |X| + Ta + Tb)(1 + u)(1 + c_z) + 4 EPS32 |silu z| (Wabs |X| + |D X|) + (u + c_z) |ref| + T
No constant comes from a measured error.  The emulation stays below 0.5 of the bound before the output's rounding and below 1 after.

Defects (each applied to `chunked` in fp64 at the library's Q; > 4 x the bound somewhere, at every length named):
    state_dropped     h is never read                                   every multi-chunk L          randn family
    tables_local      chunk c >= 1 gathers / scatters through table entries `local`, not c Q + local     "
    prev_head_state   head h reads head h - 1's state                                                  "
    state_one_chunk   h_next = update (the carry is overwritten)        L with >= 3 chunks           coherent family
    state_undecayed   h_next = h + update, without exp(s_end)                                          "
"""
import functools

import pytest
import torch

from tests.test_ssd_gpu import BF16, BIAS_H, DT_LEVEL, EPS32, F16, NAME, P, TILE, TINY, UNIT, _decay, _dual, _ratio, _silu, _softplus
from tests.test_ssd_wide_cpu import _rows, head_params, unit_gate

WIDTHS = [16, 32, 64, 128]
MAXL = 1024
SHAPES = [(2, 1), (1, 2), (3, 1), (3, 2)]                                               # (directions, batch_per_dir), by rank of L; 1024: (1, 1)
STATE_DEFECTS = ("state_one_chunk", "state_undecayed")                                  # need three chunks; coherent family
OTHER_DEFECTS = ("state_dropped", "tables_local", "prev_head_state")                   # every multi-chunk L; randn family
# added to the seed of the randn family per width, as SEED_SALT of tests/test_ssd_wide_cpu.py: chosen (if ever non-zero) by looking at
# the fp64 reference, the defect and the bound only
SEED_SALT = {16: 0, 32: 0, 64: 0, 128: 0}


@functools.lru_cache(maxsize=None)
def chunk_len(N):
    from diffma_amd import _lib

    return int(_lib.load().dm_ssd_fwd_chunk_len(N))


def lengths(N):
    Q = chunk_len(N)
    return sorted({Q + 1, 2 * Q, 2 * Q + 33, 256, MAXL})


def shape_of(L, N):
    """(directions, batch_per_dir) of a case: the four pairs by the rank of L among the width's lengths, L = 1024 a single sequence."""
    if L == MAXL:
        return (1, 1)
    ls = lengths(N)
    return SHAPES[ls.index(L) % 4] if L in ls else SHAPES[L % 4]


@functools.lru_cache(maxsize=None)
def inputs(L, dtype, N, nh=4, family="randn"):
    """Host tensors of one case: the builder of tests/test_ssd_wide_cpu.inputs (regimes cycled over the heads) with the shape from
    shape_of; family "coherent": B / C rows = a common row + 0.25 randn, x = |randn|."""
    ndir, bpd = shape_of(L, N)
    S, din = ndir * bpd, nh * P
    g = torch.Generator().manual_seed(1000 * L + 10 * nh + SEED_SALT[N] + (1 if dtype == F16 else 0) + (5 if family == "coherent" else 0))
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    reg = torch.arange(nh) % 4
    spike = (torch.arange(L)[None] + 7 * torch.arange(bpd)[:, None]) % 40 == 5
    xBC = rn(S, L, din + 2 * N)
    if family == "coherent":
        common = rn(S, 1, N) * (4.0 / N) ** 0.5
        xBC[..., :din] = xBC[..., :din].abs()
        xBC[..., din:din + N] = common + 0.25 * xBC[..., din:din + N]
        xBC[..., din + N:] = common + 0.25 * xBC[..., din + N:]
    xBC, z = xBC.to(dtype), rn(bpd, L, din).to(dtype)
    pre = torch.log(torch.expm1(DT_LEVEL[reg.clamp_max(2)] * torch.exp(0.3 * rn(bpd, L, nh))))
    ends = -12.0 + 0.3 * rn(bpd, L, nh)
    ends = torch.where(spike[..., None], (25.0 * torch.exp(0.3 * rn(bpd, L, nh))).clamp_min(20.5), ends)
    raw = torch.where(reg == 3, ends, pre)
    dt_tok = (raw - BIAS_H[reg]).to(dtype)
    zperm = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)])
    operm = torch.stack([torch.randperm(L, generator=g) for _ in range(ndir)])
    return dict(L=L, dtype=dtype, N=N, nh=nh, ndir=ndir, bpd=bpd, S=S, xBC=xBC, z=z, dt_tok=dt_tok, zperm=zperm, operm=operm)


def seq(c, s, local_Q=None):
    """fp64 operands of sequence s in scan order, as tests/test_ssd_wide_cpu.seq.  local_Q: defect tables_local -- step c Q + local
    reads (and writes) through the tables' entry `local`."""
    k, b = divmod(s, c["bpd"])
    zi, oi = c["zperm"][k], c["operm"][k]
    L, N, nh = c["L"], c["N"], c["nh"]
    if local_Q is not None:
        loc = torch.arange(L) % local_Q
        zi, oi = zi[loc], oi[loc]
    din = nh * P
    d = lambda t: t.double()
    return dict(x=d(c["xBC"][s, :, :din]).view(L, nh, P), B=d(c["xBC"][s, :, din:din + N]), C=d(c["xBC"][s, :, din + N:]),
                pre=d(c["dt_tok"][b])[zi] + head_params(nh)[2], z=d(c["z"][b])[zi].view(L, nh, P), zi=zi, oi=oi)


def chunked(q, A, D, Q, rnd=None, defect=None):
    """The kernel header's decomposition in fp64, scan order: (out, out before its rounding).  rnd: the 16-bit rounding, applied where
    the kernel rounds (the score tile, the weighted operand of the state update, the state where it is read, the output)."""
    r = rnd if rnd is not None else (lambda v: v)
    x, Bm, Cm = q["x"], q["B"], q["C"]
    L, nh, _ = x.shape
    N = Bm.shape[1]
    dt = _softplus(q["pre"])                                                             # [L, nh]
    h = torch.zeros(nh, N, P, dtype=torch.float64)
    ys = []
    for b0 in range(0, L, Q):
        sl = slice(b0, min(L, b0 + Q))
        n = sl.stop - b0
        dtc, xc, Bc, Cc = dt[sl], x[sl], Bm[sl], Cm[sl]
        s = A * dtc.cumsum(0)                                                            # chunk-local prefix sums [n, nh]
        W = r((Cc @ Bc.t())[None] * _decay(s, n) * dtc.t()[:, None, :])                  # the score tiles of the chunk, rounded once
        y = torch.einsum("hli,ihp->lhp", W, xc)
        hr = h.roll(1, 0) if defect == "prev_head_state" else h
        if defect != "state_dropped":
            y = y + torch.exp(s)[:, :, None] * torch.einsum("ln,hnp->lhp", Cc, r(hr))
        ys.append(y + D[None, :, None] * xc)
        w = dtc * torch.exp(s[-1:] - s)                                                  # [n, nh]
        upd = torch.einsum("in,ihp->hnp", Bc, r(w[:, :, None] * xc))
        if defect == "state_one_chunk":
            h = upd
        elif defect == "state_undecayed":
            h = h + upd
        else:
            h = torch.exp(s[-1])[:, None, None] * h + upd
    pre = torch.cat(ys) * _silu(q["z"])
    return r(pre), pre


def chunked_bound(q, A, D, dtype, ref_out, Q, gate=True):
    """The bound of the module docstring for one sequence (scan order).  gate False: the operator without a gate, as
    tests/test_ssd_wide_cpu.fwd_bound."""
    u, T = UNIT[dtype], TINY[dtype]
    L, N = q["B"].shape
    nh = A.shape[0]
    x, Bm, Cm, z, pre = q["x"].abs(), q["B"].abs(), q["C"].abs(), q["z"], q["pre"]
    dt = _softplus(pre)
    s = A * dt.cumsum(0)
    sT, dtT = s.t(), dt.t()
    idx = torch.arange(L)
    tl, ck = idx // TILE, idx // Q
    causal = (idx[:, None] >= idx[None, :])[None]
    M = _decay(s, L)
    Mdt = M * dtT[:, None, :]
    middle = (pre <= 20.0) & (torch.exp(pre) >= 2.0 ** -12)
    eps_dt = EPS32 * (torch.where(middle, 2.0 / dt, torch.zeros_like(dt)) + 2 * pre.abs() + 10)
    errs = (A.abs() * (eps_dt * dt).cumsum(0)).t()
    C32 = EPS32 * 12 * (sT.abs()[:, :, None] + sT.abs()[:, None, :]) + (errs[:, :, None] - errs[:, None, :]).clamp_min(0) + eps_dt.t()[:, None, :]
    Gabs = (Cm @ Bm.t())[None]
    Wabs = Gabs * Mdt
    cz = EPS32 * (2 * z.abs() + 12) if gate else torch.zeros_like(z)
    silu = _silu(z).abs() if gate else torch.ones_like(z)
    mm = lambda E, v: torch.einsum("hli,ihp->lhp", E, v)
    # ---- pairs of one chunk: tests/test_ssd_wide_cpu.fwd_bound ----
    m = torch.cat([torch.zeros(nh, 1, dtype=s.dtype), sT[:, TILE - 1::TILE], sT[:, -1:]], 1)
    alpha, gamma = torch.exp(sT - m[:, tl]), torch.exp(m[:, tl + 1] - sT)
    delta = torch.exp((m[:, tl][:, :, None] - m[:, tl + 1][:, None, :]).clamp_max(0))
    off = (tl[:, None] > tl[None, :])[None]
    P1 = torch.where(off, delta * (gamma * dtT)[:, None, :], Mdt)
    P2 = torch.where(off, delta * alpha[:, :, None], M)
    K0f = EPS32 * (72 + 2 * (N - 16) + 2 * (idx + 1.0))[None, :, None]
    E_same = ((1 + u) ** 3 - 1 + C32 + K0f) * Wabs + T * ((1 + u) ** 2 * (P1 * Bm.sum(1)[None, None, :] + P2 * Cm.sum(1)[None, :, None]) + 1 + 17 * T) * causal
    # ---- pairs whose key lies in an earlier chunk ----
    nch = (ck[:, None] - ck[None, :]).clamp_min(0)
    cross = (nch > 0)[None]
    C32x = C32 + EPS32 * 12 * sT.abs()[:, :, None]
    K0x = K0f + EPS32 * (3.0 * nch + 16)[None]
    E = torch.where(cross, ((1 + u) ** 2 - 1 + C32x + K0x) * Wabs, E_same)
    s_end = sT[:, ((ck + 1) * Q - 1).clamp_max(L - 1)]                                   # s at the end of the key's chunk [nh, L(i)]
    Mend = torch.exp((sT[:, :, None] - s_end[:, None, :]).clamp_max(0))
    Ta = T * (1 + u) * (Gabs * Mend * cross).sum(2)                                      # [nh, L]
    s_start = torch.where((ck > 0)[None], sT[:, (ck * Q - 1).clamp_min(0)], torch.zeros_like(sT))
    Tb = T * torch.exp(sT - s_start) * Cm.sum(1)[None] * (ck > 0)[None]
    Tab = (Ta + Tb).t()[:, :, None]
    Dx = D.abs()[None, :, None] * x
    return silu * (mm(E, x) + Tab) * (1 + u) * (1 + cz) + 4 * EPS32 * silu * (mm(Wabs, x) + Dx) + (u + cz) * ref_out.abs() + T


@functools.lru_cache(maxsize=None)
def analysis(L, dtype, N, nh=4, family="randn", gate=True):
    """(ref, tol) [S, L, nh * P] of one case in the kernel's output layout: the fp64 dual form and its bound.  Computed once per case.
    gate False: the same operands without the gate, out = Y + D x."""
    c = inputs(L, dtype, N, nh, family)
    A, D, _ = head_params(nh)
    Q = chunk_len(N)
    ref, tol = [], []
    for s in range(c["S"]):
        q = seq(c, s)
        if not gate:
            q = {**q, "z": torch.full_like(q["z"], unit_gate())}
        out = _dual(q, A, D)
        ref.append(_rows(out, q["oi"], L))
        tol.append(_rows(chunked_bound(q, A, D, dtype, out, Q, gate), q["oi"], L))
    return torch.stack(ref), torch.stack(tol)


def _emulation(L, dtype, N, family="randn"):
    c = inputs(L, dtype, N, 4, family)
    A, D, _ = head_params(4)
    rnd = lambda v: v.to(dtype).double()
    out, pre = [], []
    for s in range(c["S"]):
        q = seq(c, s)
        o, p_ = chunked(q, A, D, chunk_len(N), rnd=rnd)
        out.append(_rows(o, q["oi"], L))
        pre.append(_rows(p_, q["oi"], L))
    return torch.stack(out), torch.stack(pre)


def _defective(L, dtype, N, defect, family):
    c = inputs(L, dtype, N, 4, family)
    A, D, _ = head_params(4)
    Q = chunk_len(N)
    res = []
    for s in range(c["S"]):
        if defect == "tables_local":
            q = seq(c, s, local_Q=Q)
            o = chunked(q, A, D, Q)[0].reshape(L, -1)
            rows = torch.zeros_like(o)
            for b0 in range(0, L, Q):                                                    # chunks in order: a later one overwrites the rows of an earlier one
                sl = slice(b0, min(L, b0 + Q))
                rows[q["oi"][sl]] = o[sl]
            res.append(rows)
        else:
            q = seq(c, s)
            res.append(_rows(chunked(q, A, D, Q, defect=defect)[0], q["oi"], L))
    return torch.stack(res)


def defect_lengths(N, defect):
    Q = chunk_len(N)
    return [L for L in lengths(N) if L > (2 * Q if defect in STATE_DEFECTS else Q)]


# =====================================================================================================================================
def test_supported_set_of_the_chunked_entry():
    """The C ABI's answers: every width in both 16-bit dtypes for 1 <= L <= 1024, nothing else; the chunk length per width; the
    single-chunk entry's answer at 225 unchanged; the ABI version."""
    from diffma_amd import _lib, hip_ops

    lib = _lib.load()
    bf16, f16, f32 = _lib.DM_BF16, _lib.DM_F16, _lib.DM_F32
    for code in (bf16, f16):
        for N in WIDTHS:
            for L in (1, 224, 225, 256, 1024):
                assert lib.dm_ssd_fwd_chunked_supported(L, 64, N, code) == 1, (L, N, code)
            for L in (0, 1025):
                assert lib.dm_ssd_fwd_chunked_supported(L, 64, N, code) == 0, (L, N, code)
            assert lib.dm_ssd_fwd_chunked_supported(256, 32, N, code) == 0
            assert lib.dm_ssd_fwd_supported(225, 64, N, code) == 0
        for N in (8, 24, 48, 256):
            assert lib.dm_ssd_fwd_chunked_supported(256, 64, N, code) == 0, (N, code)
    for N in WIDTHS:
        assert lib.dm_ssd_fwd_chunked_supported(256, 64, N, f32) == 0
        Q = lib.dm_ssd_fwd_chunk_len(N)
        assert Q % 32 == 0 and 64 <= Q <= 224, (N, Q)
    for N in (0, 8, 24, 48, 256):
        assert lib.dm_ssd_fwd_chunk_len(N) <= 0
    assert lib.dm_abi_version() >= 34 and _lib.CONSTANTS["DM_ABI_VERSION"] >= 34 and _lib.CONSTANTS["DM_SSD_FWD_CHUNKED_MAXL"] == MAXL
    assert all(lib.dm_ssd_fwd_chunked_supported(1024, 64, N, bf16) == 1 for N in hip_ops.SSD_FWD_CHUNKED_WIDTHS)
    assert isinstance(hip_ops.SSD_CHUNKED, bool)


@pytest.mark.parametrize("N", WIDTHS)
def test_chunked_restatement_equals_the_dual_form(N):
    """The decomposition of the kernel header in fp64, at the library's chunk length and L = 2 Q + 33 (three chunks, the last one
    ragged), against the chunk-free dual form: 1e-12 relative to the largest output, all head regimes."""
    Q = chunk_len(N)
    L = 2 * Q + 33
    c = inputs(L, BF16, N)
    A, D, _ = head_params(4)
    for s in range(c["S"]):
        q = seq(c, s)
        ref, got = _dual(q, A, D), chunked(q, A, D, Q)[0]
        for h in range(4):
            err = float((got[:, h] - ref[:, h]).abs().max() / ref[:, h].abs().max())
            assert err <= 1e-12, (N, s, h, err)


@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_chunked_bound_holds_for_the_emulation_with_margin(dtype, N):
    """The bound against the emulation: <= 0.5 for `out` before its last rounding, <= 1 after it, at every length, both families."""
    worst = {"out": 0.0, "out_pre": 0.0}
    for family, Ls in (("randn", lengths(N)), ("coherent", defect_lengths(N, "state_one_chunk"))):
        for L in Ls:
            ref, tol = analysis(L, dtype, N, 4, family)
            out, pre = _emulation(L, dtype, N, family)
            r, rp = float(_ratio(out, ref, tol).max()), float(_ratio(pre, ref, tol).max())
            worst = {"out": max(worst["out"], r), "out_pre": max(worst["out_pre"], rp)}
            assert rp <= 0.5 and r <= 1.0, (family, L, N, NAME[dtype], rp, r)
    print(N, NAME[dtype], {k: round(v, 4) for k, v in worst.items()})


@pytest.mark.parametrize("defect", OTHER_DEFECTS + STATE_DEFECTS)
@pytest.mark.parametrize("N", WIDTHS)
@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_chunked_bound_tells_each_defect_from_the_reference(dtype, N, defect):
    """Each defect leaves at least one element more than 4 x its bound away from the reference at every length named for it; the
    coherent family stays inside |out| < 4096."""
    family = "coherent" if defect in STATE_DEFECTS else "randn"
    seen = {}
    for L in defect_lengths(N, defect):
        ref, tol = analysis(L, dtype, N, 4, family)
        assert family != "coherent" or float(ref.abs().max()) < 4096.0, float(ref.abs().max())
        seen[L] = float(_ratio(_defective(L, dtype, N, defect, family), ref, tol).max())
    print(defect, N, NAME[dtype], {L: round(v, 1) for L, v in seen.items()})
    assert seen and all(v > 4.0 for v in seen.values()), (defect, N, NAME[dtype], seen)
