"""The selective-scan kernels on the device, every element inside the fp64 bounds of tests/test_scan_bounds_cpu.py (reference, rounding
places, constants and the defect catalogue are derived there; nothing here is fitted to a measured error).

Every test asserts through the launch queries (scan_fwd_segment, scan_bwd_segment, dm_scan_bwd_launch_group_channels) that the family it
names is the one that ran, and forces `variant=` where the library would choose otherwise.  u | delta | z are column blocks of one
NaN-padded buffer; out, du, ddelta and dz are views inside sentinel frames that start as NaN: every element must be written, inside its
bound, and the frame must survive bit for bit.  The dB/dC partial rows and the dA | dD | dbias partials start as NaN as well.

Shapes (the smallest at which each form can go wrong; S <= 6):
  K2   d_state 16: L 1 (one step), 4 (slot 0 after one sub-chunk), 5 (one valid step in a ragged sub-chunk), 8 (slot 0 on a chunk boundary),
       11 (L % 4 = 3), 29 (four staging chunks, both bc_lds buffers), 196; Dm 72 (a full wave, an 8-lane wave, two idle waves) and 320 (two
       workgroups, the second ragged); every call pattern at L 11 and 29; d_state 8 / 32 at Dm 200 and 64 / 128 at Dm 96, plain and with tables;
       the one-exp form at 16, 64, 128.
  K2c  L 17, 20, 56 (7 waves x 8 steps) and 57, 60, 183, 196 (7 x 28), Dm 72, the call patterns at 20 and 60; a congruent pair through
       dm_selective_scan_bwd_n, each struct against its own bound.
  K1   L 1, 7, 8, 9, 17, 196, Dm 72 / 200, with and without checkpoints, EVERY checkpoint slot and last_state per element, the accumulating
       three-direction form, d_state 8 / 32 / 64 / 128 (the split-channel forms among them), ngroups = 2 at 64 and 128 channels per group.
  K1c  L 57 (the shortest the query reports), 100, 183, 196, with and without checkpoints, ngroups = 2.
The forward that writes a backward case's checkpoints is checked too (out and every slot).

Worst |got - ref| / bound per (family, output, dtype / d_state), 2026-10-21, one MI355X ("K2 fwd" / "K2c fwd": the forward that wrote a
backward case's checkpoints; f32 / 64 ran as well: within 0.92 everywhere).  No bound term was added after the first device run.
  family   output      bf16/16   f16/16   f32/16   bf16/8    f16/8  bf16/32   f16/32  bf16/64   f16/64 bf16/128  f16/128
  K1       ckpt          0.995    0.980    0.933    0.980    0.840    0.988    0.900    0.995    0.904    0.996    0.918
  K1       last_state    0.966    0.980    0.647    0.521    0.505    0.600    0.629    0.652    0.621    0.673    0.666
  K1       out           0.995    0.986    0.672    0.989    0.961    0.937    0.960    0.964    0.971    0.928    0.945
  K1c      ckpt          0.994    0.929    0.923        -        -        -        -        -        -        -        -
  K1c      out           0.993    0.987    0.518        -        -        -        -        -        -        -        -
  K2 fwd   ckpt          0.996    0.947    0.883    0.994    0.942    0.995    0.926    0.995    0.954    0.996    0.949
  K2 fwd   last_state    0.957    0.915    0.510    0.741    0.717    0.802    0.766    0.750    0.748    0.796    0.791
  K2 fwd   out           0.994    0.986    0.631    0.993    0.992    0.992    0.982    0.986    0.974    0.978    0.967
  K2       dA            0.978    0.722    0.291    0.966    0.634    0.970    0.539    0.957    0.515    0.979    0.621
  K2       dB            0.617    0.224    0.200    0.385    0.071    0.369    0.124    0.218    0.274    0.322    0.346
  K2       dC            0.681    0.217    0.158    0.334    0.079    0.374    0.091    0.658    0.146    0.725    0.206
  K2       dD            0.228    0.198    0.029    0.083    0.086    0.104    0.136    0.107    0.112    0.099    0.070
  K2       dbias         0.458    0.332    0.085    0.404    0.218    0.216    0.197    0.204    0.158    0.125    0.158
  K2       ddelta        0.990    0.979    0.481    0.982    0.955    0.977    0.947    0.975    0.920    0.959    0.874
  K2       du            0.995    0.998    0.892    0.996    0.989    0.995    0.990    0.994    0.984    0.989    0.993
  K2       dz            0.994    0.992    0.607    0.988    0.986    0.995    0.988    0.984    0.956    0.977    0.969
  K2c fwd  ckpt          0.996    0.941    0.904        -        -        -        -        -        -        -        -
  K2c fwd  last_state    0.651    0.620        -        -        -        -        -        -        -        -        -
  K2c fwd  out           0.996    0.993    0.491        -        -        -        -        -        -        -        -
  K2c      dA            0.958    0.447    0.136        -        -        -        -        -        -        -        -
  K2c      dB            0.721    0.205    0.179        -        -        -        -        -        -        -        -
  K2c      dC            0.661    0.179    0.148        -        -        -        -        -        -        -        -
  K2c      dD            0.053    0.058    0.009        -        -        -        -        -        -        -        -
  K2c      dbias         0.226    0.195    0.043        -        -        -        -        -        -        -        -
  K2c      ddelta        0.982    0.972    0.489        -        -        -        -        -        -        -        -
  K2c      du            0.996    0.992    0.874        -        -        -        -        -        -        -        -
  K2c      dz            0.992    0.984    0.442        -        -        -        -        -        -        -        -
  K2c pair dA            0.865    0.239        -        -        -        -        -        -        -        -        -
  K2c pair dB            0.661    0.206        -        -        -        -        -        -        -        -        -
  K2c pair dC            0.482    0.201        -        -        -        -        -        -        -        -        -
  K2c pair dD            0.025    0.023        -        -        -        -        -        -        -        -        -
  K2c pair dbias         0.119    0.127        -        -        -        -        -        -        -        -        -
  K2c pair ddelta        0.957    0.951        -        -        -        -        -        -        -        -        -
  K2c pair du            0.995    0.985        -        -        -        -        -        -        -        -        -
  K2c pair dz            0.993    0.974        -        -        -        -        -        -        -        -        -
"""
import pytest
import torch

from tests.test_mixer_passes_gpu import _frame, _intact
from tests.test_scan_bounds_cpu import BF16, F16, F32, PATTERNS, SUB, bwd_cases, bwd_cases_wide, case, check, cid, fwd_cases, inputs, report

pytestmark = pytest.mark.gpu
NAN = float("nan")
SEQ, CHUNKED = 16, 32                                   # DM_FLAG_SCAN_SEQUENTIAL, DM_FLAG_SCAN_CHUNKED


def _framed(gpu, dt, S, L, Dm):
    sl = Dm + 8
    return _frame(gpu, dt, (S, L, Dm), (L * sl + 8, sl, 1), 8)


def _operands(gpu, c):
    """Device operands of a case: u | delta | z as column blocks of a NaN-padded buffer (z apart when the directions share it)."""
    t = inputs(c)
    S, L, Dm = c.ndir * c.bpd, c.L, c.Dm
    shared_z = c.z and t["z"].shape[0] != S
    buf = torch.full((S, L + 2, 3 * Dm + 8), NAN, dtype=c.dtype, device=gpu)
    v = buf[:, 1:L + 1]
    o = dict(keep=buf, u=v[..., :Dm], delta=v[..., Dm:2 * Dm], z=None)
    o["u"].copy_(t["u"])
    o["delta"].copy_(t["delta"])
    if c.z and not shared_z:
        o["z"] = v[..., 2 * Dm:3 * Dm]
        o["z"].copy_(t["z"])
    elif c.z:
        zb = torch.full((c.bpd, L + 2, Dm + 8), NAN, dtype=c.dtype, device=gpu)
        o["z"] = zb[:, 1:L + 1, :Dm]
        o["z"].copy_(t["z"])
    bc = (lambda x: x.float()) if c.bcf32 else (lambda x: x)
    o.update(A=t["A"].to(gpu), D=t["D"].to(gpu), bias=None if t["bias"] is None else t["bias"].to(gpu), B=bc(t["B"]).to(gpu), C=bc(t["C"]).to(gpu),
             dout=t["dout"].to(gpu))
    o["tabs"] = dict(z_row_index=t["zperm"].int().to(gpu), out_row_index=t["operm"].int().to(gpu), batch_per_dir=c.bpd) if c.tables else {}
    return o


def _flags(c, variant):
    return (1 if c.mode == 1 else 0) | (8 if c.ash else 0) | (128 if c.mode == 2 else 0) | {"sequential": SEQ, "chunked": CHUNKED}[variant]


def _ckpt_states(ho, ck, c):
    """Checkpoint buffer -> fp32 states [S, slots, N, Dm] (packed bf16: word w of (group g, channel d) = states 8 g + 2 w | 8 g + 2 w + 1)."""
    if ck.dtype != torch.int32:
        return ck.float()
    S, nck = ck.shape[:2]
    w = ck.view(S, nck, c.N // 8, c.Dm, 4)
    lo, hi = (w << 16).view(torch.float32), (w & -65536).view(torch.float32)
    return torch.stack([lo, hi], -1).permute(0, 1, 2, 4, 5, 3).reshape(S, nck, c.N, c.Dm)


def _forward(gpu, c, variant, o=None, with_ckpt=None, what=None):
    """Runs the forward of a case in the named family and checks out, every checkpoint slot and (K1) last_state.  Returns (operands, ckpt)."""
    from diffma_amd import hip_ops as ho

    o = o or _operands(gpu, c)
    S, L, Dm, N = c.ndir * c.bpd, c.L, c.Dm, c.N
    with_ckpt = c.ckpt if with_ckpt is None else with_ckpt
    seg = ho.scan_fwd_segment(S, Dm, L, N, _flags(c, variant))
    assert (seg == 196) if variant == "chunked" else (seg == 0), (variant, seg)
    ck = None
    if with_ckpt:
        ck = ho.alloc_scan_ckpt(S, L, N, Dm, c.dtype, gpu)
        ck.view(torch.int32).fill_(0x7FC07FC0)                       # NaN in either format: every slot must be written
    obuf, out = _framed(gpu, c.dtype, c.bpd if c.acc else S, L, Dm)
    last = torch.full((S, N, Dm), NAN, device=gpu) if (variant == "sequential" and not c.acc and c.mode != 2) else None
    res = ho.scan_fwd(o["u"], o["delta"], o["A"], o["B"], o["C"], o["D"], o["z"], o["bias"], c.mode == 1, out=out, ckpt=ck, last_state=last,
                      ngroups=c.groups, a_shared=c.ash, variant=None if c.acc else variant, acc_dirs=c.acc, delta_activated=c.mode == 2, **o["tabs"])
    torch.cuda.synchronize()
    assert res.data_ptr() == out.data_ptr()
    _intact(obuf, out, "scan_fwd out")
    what = what or ("K1" if variant == "sequential" else "K1c")
    check(c, "out", out.float().cpu(), what)
    if ck is not None:
        check(c, "ckpt", _ckpt_states(ho, ck, c).cpu(), what)
    if last is not None:
        check(c, "last_state", last.cpu(), what)
    return o, ck


def _bwd_struct(gpu, c, o, ck, variant):
    """dm_scan_bwd_args as hip_ops.scan_bwd builds it, with EVERY output a NaN view in a sentinel frame or a NaN buffer."""
    from diffma_amd import hip_ops as ho

    S, L, Dm, N = c.ndir * c.bpd, c.L, c.Dm, c.N
    A32, D32, b32 = ho._f32c(o["A"]), ho._f32c(o["D"]), ho._f32c(o["bias"])
    tabs = o["tabs"]
    a = ho._scan_args(ho.dm_scan_bwd_args(), o["u"], o["delta"], A32, o["B"], o["C"], D32, o["z"], b32, c.mode == 1, c.mode == 2,
                      tabs.get("z_row_index"), tabs.get("out_row_index"), tabs.get("batch_per_dir", 0), ck, SUB, 1, c.ash, None,
                      {"sequential": SEQ, "chunked": CHUNKED}[variant] | (4 if c.dps else 0))
    shape = ho.scan_bwd_partial_shape(S, L, Dm, N, a.flags)
    r = dict(keep=[A32, D32, b32], a=a, nw=shape[2])
    r["dubuf"], r["du"] = _framed(gpu, c.dtype, S, L, Dm)
    r["ddbuf"], r["ddelta"] = _framed(gpu, c.dtype, S, L, Dm)
    if c.z:
        r["dzbuf"], r["dz"] = _framed(gpu, c.dtype, S, L, Dm)
    r["dBC"] = torch.full(shape, NAN, device=gpu)
    pcols = Dm * N + 2 * Dm
    r["part"] = torch.full((S, pcols), NAN, device=gpu)
    a.part_ss = pcols
    a.dout = o["dout"].data_ptr()
    a.du, a.ddelta, a.dz = r["du"].data_ptr(), r["ddelta"].data_ptr(), (r["dz"].data_ptr() if c.z else 0)
    a.dBC_partial, a.dA_partial = r["dBC"].data_ptr(), r["part"].data_ptr()
    a.dD_partial, a.dbias_partial = r["part"][:, Dm * N:].data_ptr(), r["part"][:, Dm * N + Dm:].data_ptr()
    if c.z:
        a.dz_ss, a.dz_sl, a.dz_sd = r["dz"].stride()
    a.do_ss, a.do_sl, a.do_sd = o["dout"].stride()
    a.du_ss, a.du_sl, a.du_sd = r["du"].stride()
    a.ddt_ss, a.ddt_sl, a.ddt_sd = r["ddelta"].stride()
    return r


def _bwd_finish(gpu, c, r, what):
    from diffma_amd import hip_ops as ho

    S, L, Dm, N = c.ndir * c.bpd, c.L, c.Dm, c.N
    torch.cuda.synchronize()
    for k in ("du", "ddelta") + (("dz",) if c.z else ()):
        _intact(r[k[:2] + "buf"], r[k], f"scan_bwd {k}")
        check(c, k, r[k].float().cpu(), what)
    dBC = ho.sum_partials(r["dBC"].view(S * L, r["nw"], 2 * N), torch.empty((S, L, 2 * N), dtype=torch.float32, device=gpu)).cpu()
    check(c, "dB", dBC[..., :N], what)
    check(c, "dC", dBC[..., N:], what)
    ps = ho.colsum(r["part"]).cpu()
    check(c, "dA", ps[:Dm * N].view(Dm, N), what)
    check(c, "dD", ps[Dm * N:Dm * N + Dm], what)
    check(c, "dbias", ps[Dm * N + Dm:], what)


def _fwd_variant_for(c):
    """The forward that writes a backward case's checkpoints: K2c's model patterns past 56 tokens take K1c as the model does, all else K1."""
    model = c.tables and ((c.z and c.mode == 1) or (not c.z and c.mode != 1))
    return "chunked" if (c.fam == "K2c" and c.L > 56 and model) else "sequential"


def _backward(gpu, c):
    from diffma_amd import _lib, hip_ops as ho

    S, L, Dm, N = c.ndir * c.bpd, c.L, c.Dm, c.N
    variant = "sequential" if c.fam == "K2" else "chunked"
    o, ck = _forward(gpu, c, _fwd_variant_for(c), with_ckpt=True, what=c.fam + " fwd")
    r = _bwd_struct(gpu, c, o, ck, variant)
    seg = ho.scan_bwd_segment(S, Dm, L, N, r["a"].flags)
    gc = _lib.load().dm_scan_bwd_launch_group_channels(S, Dm, L, N, r["a"].flags)
    if c.fam == "K2":
        assert seg == 0 and gc == {8: 256, 16: 256, 32: 128, 64: 64, 128: 32}[N], (seg, gc)
    else:
        assert seg == (56 if L <= 56 else 196) and gc == 64, (seg, gc)
    ho._launch("dm_selective_scan_bwd", r["a"], o["u"], 0)
    _bwd_finish(gpu, c, r, c.fam)


BWD = [c for dt in (BF16, F16) for c in bwd_cases(dt)] + [case("K2", F32, 29, 72, seed=30, **PATTERNS["three_dirs"]),
                                                          case("K2c", F32, 60, 72, seed=30, **PATTERNS["three_dirs"])]
WIDE = [c for dt in (BF16, F16) for c in bwd_cases_wide(dt)] + [case("K2", F32, 29, 96, N=64, seed=31, **PATTERNS["three_dirs"])]
FWD = [c for dt in (BF16, F16) for c in fwd_cases(dt)] + [case("K1", F32, 17, 72, seed=32, **PATTERNS["three_dirs"]),
                                                          case("K1c", F32, 100, 72, seed=32, **PATTERNS["three_dirs"])]


@pytest.mark.parametrize("c", BWD, ids=cid)
def test_scan_bwd_within_derived_bound(gpu, c):
    """K2 / K2c at d_state 16: du, ddelta, dz, dB, dC, dA, dD, dbias (and the forward of the same launch) per element inside the bound."""
    _backward(gpu, c)


@pytest.mark.parametrize("c", WIDE, ids=cid)
def test_scan_bwd_other_widths_within_derived_bound(gpu, c):
    """K2 at d_state 8 / 32 (bf16: the non-HALVES matrix-pipe sum; 32: two lanes per channel) and 64 / 128 (permlane sums in every dtype,
    4 and 8 lanes per channel), plain and with tables; the one-exp form at 64 and 128."""
    _backward(gpu, c)


@pytest.mark.parametrize("c", FWD, ids=cid)
def test_scan_fwd_within_derived_bound(gpu, c):
    """K1 / K1c: out, every checkpoint slot and last_state per element; the accumulating form; the other widths; ngroups = 2."""
    _forward(gpu, c, "sequential" if c.fam == "K1" else "chunked")


@pytest.mark.parametrize("dtype", [BF16, F16], ids=["bf16", "f16"])
def test_scan_bwd_pair_each_struct_within_its_bound(gpu, dtype):
    """Two congruent structs (different values) through dm_selective_scan_bwd_n share one K2c launch; each is held to its OWN bound."""
    from diffma_amd import _lib, hip_ops as ho

    cs = [case("K2c", dtype, 20, 72, seed=s, **PATTERNS["three_dirs"]) for s in (40, 41)]
    rs = []
    for c in cs:
        o, ck = _forward(gpu, c, "sequential", with_ckpt=True, what="K2c fwd")
        rs.append((o, ck, _bwd_struct(gpu, c, o, ck, "chunked")))
    assert ho.scan_bwd_segment(6, 72, 20, 16, rs[0][2]["a"].flags) == 56
    _lib.call_n("dm_selective_scan_bwd", [r[2]["a"] for r in rs], torch.cuda.current_stream().cuda_stream)
    for c, r in zip(cs, rs):
        _bwd_finish(gpu, c, r[2], "K2c pair")


def test_zz_error_to_bound_ratios():
    report()
