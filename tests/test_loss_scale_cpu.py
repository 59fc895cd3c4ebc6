"""The loss scale of the graphed fp16 training step (csrc/optim.hip: dm_adamw_args.grad_scale, dm_loss_scale_update; optim.DeviceLossScale):
the parts that need no GPU.  tests/test_loss_scale_gpu.py imports the update rule, the scaled-gradient builders and the bound from here.

The update rule (`update_rule`) is torch._amp_update_scale_ written out on the host: the scale is an fp32 value, factor products are taken
in double and rounded once to fp32, a growth whose product is not finite is not applied (the tracker still returns to 0), and the tracker
only ever triggers on EQUALITY with the interval.

AdamW with a gradient scale.  The device holds gs; the kernel forms gq = (float)((double)gs / (double)scale) and goes on as before.
  * scale = 2^k and gs = g 2^k with g and gs both in fp32's normal range (or 0): gq == g bit for bit, so the outputs must pass the existing
    aw_eval of the unscaled case unchanged (`aws_pow2_case` asserts the range, so the exactness claim cannot fail silently).
  * any other scale: the reference is fp64 with the fp64 quotient q = gs / scale, and gq = q (1 + d), |d| <= E = 2^-24 (one rounding; F =
    2^-100 absolute covers a quotient in the denormal range): d_g = E |q| + F.  It propagates through the header's formulas, on top of the
    existing bounds of test_step_kernels_cpu (quoted as "base"):
        m = b1 m0 + (1 - b1) q:           d_m = base + (1 - b1) d_g
        v = b2 v0 + (1 - b2) q^2:         d_v = base + (1 - b2) (2 |q| d_g + d_g^2)
        sq = sqrt(v) / sqrt(bc2):         x_sq = min(x_v / sqrt(v), sqrt(x_v)) / sqrt(bc2)     (x_ = the part added here; |sqrt a - sqrt b| is
                                          at most |a - b| / sqrt(max(a, b)) and at most sqrt|a - b|)
        den = sq + eps:                   d_den = base + x_sq
        upd = ss m / den:                 d_upd = base + (ss x_m + |upd| x_sq) / (den - x_sq)   (the perturbed denominator, written out)
        p = pw - upd, ema:                the existing expressions with the larger d_upd / d_p.
    `aws_eval` is aw_eval's accepted-step arm with these terms; test_scaled_emulation_meets_the_bound checks it against the fp32
    emulation (aw_emul on the rounded quotient) before the GPU file relies on it.  Largest ratio of the emulation: 0.986 at both scales.
"""
import math
from types import SimpleNamespace as NS

import pytest
import torch

from tests.test_mixer_passes_cpu import EPS32, F32, FLOOR, bits_equal
from tests.test_step_kernels_cpu import F64, INF, aw_case, aw_emul, aw_eval, aw_hp, judge, ratio

E = EPS32
POW2_SCALES = [1.0, 2.0 ** 16, 2.0 ** -3]
ODD_SCALES = [3.0, 1000.0]
F32_MIN_NORMAL, F32_MAX = 2.0 ** -126, 3.4028234663852886e38


def f32(x):
    """A double rounded once to fp32, returned as a Python float (Inf past fp32's range)."""
    return float(torch.tensor(x, dtype=F64).float())


def update_rule(scale, tracker, found, growth=2.0, backoff=0.5, interval=2000):
    """(scale, tracker) after one torch._amp_update_scale_; `scale` is an fp32 value held in a Python float."""
    if found != 0.0:
        return f32(scale * backoff), 0
    successful = tracker + 1
    if successful == interval:
        grown = f32(scale * growth)
        return (grown if math.isfinite(grown) else scale), 0
    return scale, successful


BIG = f32(3e38)
# (scale, tracker, found, growth, backoff, interval) -> (scale, tracker), worked out by hand
RULE_TABLE = [
    ((65536.0, 0, 1.0, 2.0, 0.5, 2000), (32768.0, 0)),                      # back-off
    ((65536.0, 1234, 1.0, 2.0, 0.5, 2000), (32768.0, 0)),                   # ... forgets the clean steps counted so far
    ((65536.0, 5, 0.0, 2.0, 0.5, 2000), (65536.0, 6)),                      # a clean step is counted
    ((65536.0, 1998, 0.0, 2.0, 0.5, 2000), (65536.0, 1999)),                # one short of the interval
    ((65536.0, 1999, 0.0, 2.0, 0.5, 2000), (131072.0, 0)),                  # growth
    ((BIG, 1999, 0.0, 2.0, 0.5, 2000), (BIG, 0)),                           # 6e38 is not an fp32: no growth, the tracker still restarts
    ((BIG, 0, 0.0, 2.0, 0.5, 1), (BIG, 0)),                                 # the same guard at interval 1
    ((BIG, 2, 0.0, 1.125, 0.5, 3), (f32(3e38 * 1.125), 0)),                 # 3.375e38 still fits
    ((1.0, 0, 0.0, 2.0, 0.5, 1), (2.0, 0)),                                 # interval 1: every clean step grows
    ((1.0, 0, 1.0, 2.0, 0.5, 1), (0.5, 0)),
    ((1.0, -1, 0.0, 2.0, 0.5, 1), (1.0, 0)),                                # the trigger is equality with the interval
    ((1.0, 5, 0.0, 2.0, 0.5, 3), (1.0, 6)),                                 # ... so a tracker past it just counts on
    ((1.0, 2, 0.0, 1.5, 0.3, 3), (1.5, 0)),
    ((1.0, 2, 1.0, 1.5, 0.3, 3), (0.30000001192092896, 0)),                 # (float)0.3: the product is rounded to fp32
    ((65536.0, 1, 1.0, 1.5, 0.3, 3), (19660.80078125, 0)),                  # 65536 * 0.3 = 19660.8 -> nearest fp32 (spacing 2^-9)
    ((2.0 ** -120, 0, 1.0, 2.0, 0.5, 3), (2.0 ** -121, 0)),
    ((2.0 ** -120, 2, 0.0, 2.0, 0.5, 3), (2.0 ** -119, 0)),
]


def test_update_rule_against_a_hand_written_table():
    assert abs(BIG / 3e38 - 1) <= 2 ** -24
    assert math.isinf(f32(BIG * 2.0)) and math.isfinite(f32(BIG * 1.125))
    for args, want in RULE_TABLE:
        assert update_rule(*args) == want, (args, update_rule(*args), want)
    # interval 1 over a sequence: grows on every clean step, halves on every found one
    s, t, seen = 1.0, 0, []
    for found in (0.0, 0.0, 1.0, 0.0, 1.0, 1.0):
        s, t = update_rule(s, t, found, interval=1)
        seen.append((s, t))
    assert seen == [(2.0, 0), (4.0, 0), (2.0, 0), (4.0, 0), (2.0, 0), (1.0, 0)]


def test_update_rule_is_torch_amp_update_scale_on_the_cpu():
    """The same table and a random walk through torch's own CPU kernel, bit for bit."""
    def torch_rule(scale, tracker, found, growth, backoff, interval):
        s, t, f = torch.tensor([scale], dtype=F32), torch.tensor([tracker], dtype=torch.int32), torch.tensor([found], dtype=F32)
        torch._amp_update_scale_(s, t, f, growth, backoff, interval)
        return float(s), int(t)

    for args, want in RULE_TABLE:
        assert torch_rule(*args) == want, args
    g = torch.Generator().manual_seed(3)
    s = ts = 65536.0
    t = tt = 0
    for k in range(200):
        found = float(torch.rand((), generator=g) < 0.2)
        s, t = update_rule(s, t, found, 1.5, 0.3, 3)
        ts, tt = torch_rule(ts, tt, found, 1.5, 0.3, 3)
        assert (s, t) == (ts, tt), k


def test_abi_names_the_loss_scale():
    from diffma_amd import _lib

    lib = _lib.load()
    assert lib.dm_abi_version() >= 37 and _lib.CONSTANTS["DM_ABI_VERSION"] >= 37
    assert "dm_loss_scale_update" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "dm_loss_scale_update")
    import ctypes
    assert _lib.ARGTYPES["dm_loss_scale_update"] == [ctypes.c_void_p, ctypes.c_void_p]


def test_structs_parse_from_the_header():
    import ctypes

    from diffma_amd import _lib

    P, D, I = ctypes.c_void_p, ctypes.c_double, ctypes.c_int32
    assert _lib.STRUCT_FIELDS["dm_loss_scale_args"] == [("scale", P), ("growth_tracker", P), ("found_inf", P), ("skipped", P),
                                                        ("growth_factor", D), ("backoff_factor", D), ("growth_interval", I)]
    aw = _lib.STRUCT_FIELDS["dm_adamw_args"]
    assert aw[-1] == ("grad_scale", P) and aw[-2] == ("nonfinite_out", P)
    assert [n for n, _ in aw].count("grad_scale") == 1
    # appended: every earlier field keeps its offset, and a zero-initialised struct has no scale
    a = _lib.dm_adamw_args()
    assert not a.grad_scale
    assert type(a).grad_scale.offset == type(a).nonfinite_out.offset + 8 and ctypes.sizeof(a) == type(a).grad_scale.offset + 8


def test_state_dict_round_trip_with_grad_scaler():
    """optim.scale_state_dict / scale_state_parse (what DeviceLossScale.state_dict / load_state_dict go through) against the public
    format of torch.amp.GradScaler, both directions."""
    from diffma_amd import optim

    sd = optim.scale_state_dict(1024.0, 1.5, 0.3, 7, 4)
    assert list(sd) == ["scale", "growth_factor", "backoff_factor", "growth_interval", "_growth_tracker"]
    ref = torch.amp.GradScaler("cpu")
    assert set(ref.state_dict()) == set(sd)
    ref.load_state_dict(sd)
    back = ref.state_dict()
    assert back == sd and all(type(back[k]) is type(sd[k]) for k in sd), (back, sd)
    assert ref.get_growth_factor() == 1.5 and ref.get_backoff_factor() == 0.3 and ref.get_growth_interval() == 7
    theirs = torch.amp.GradScaler("cpu", init_scale=4096.0, growth_factor=3.0, backoff_factor=0.25, growth_interval=11).state_dict()
    assert optim.scale_state_parse(theirs) == (4096.0, 3.0, 0.25, 11, 0)
    assert optim.scale_state_dict(*optim.scale_state_parse(theirs)[:4], 0) == theirs
    with pytest.raises(KeyError):
        optim.scale_state_parse({})                                         # a disabled GradScaler's state dict
    with pytest.raises(KeyError):
        optim.scale_state_parse({k: v for k, v in sd.items() if k != "_growth_tracker"})


def test_device_loss_scale_defaults_are_grad_scalers():
    import inspect

    from diffma_amd import optim

    ours = inspect.signature(optim.DeviceLossScale.__init__).parameters
    theirs = inspect.signature(torch.amp.GradScaler.__init__).parameters
    for k in ("init_scale", "growth_factor", "backoff_factor", "growth_interval"):
        assert ours[k].default == theirs[k].default, k
    for bad in (dict(growth_factor=0.0), dict(backoff_factor=-1.0), dict(growth_factor=INF), dict(growth_interval=0)):
        with pytest.raises(ValueError):
            optim.DeviceLossScale("cpu", **bad)
    if torch.cuda.is_available():
        a = optim.DeviceLossScale("cuda", init_scale=512.0, growth_interval=5)
        gs = torch.amp.GradScaler("cuda")
        gs.load_state_dict(a.state_dict())
        assert gs.state_dict() == a.state_dict()
        b = optim.DeviceLossScale("cuda")
        b.load_state_dict(gs.state_dict())
        assert b.state_dict() == a.state_dict() and b.scale.dtype == F32 and b.growth_tracker.dtype == torch.int32 and b.scale.dim() == 0


# =====================================================================================================================================
# dm_adamw_ema_step with grad_scale
# =====================================================================================================================================
def _with_g(c, fn):
    return NS(ts=[NS(n=T.n, p=T.p, m=T.m, v=T.v, g=fn(T.g), ema=T.ema, step=T.step) for T in c.ts], chunk=c.chunk, bt=c.bt, bc=c.bc)


def aws_pow2_case(c, scale):
    """Case c with every gradient multiplied by the power of two `scale`: exact, and asserted to be."""
    assert math.frexp(scale)[0] == 0.5
    out = _with_g(c, lambda g: (g.double() * scale).float())
    for T, S in zip(c.ts, out.ts):
        for x in (T.g, S.g):
            a = x.double().abs()
            assert bool(((a == 0) | ((a >= F32_MIN_NORMAL) & (a <= F32_MAX))).all()), "a gradient leaves fp32's normal range"
        assert bool((S.g.double() / scale == T.g.double()).all()) and bool(((S.g == 0) == (T.g == 0)).all())
    return out


def aws_quotient_case(c, scale):
    """The case the kernel effectively works on: every gradient replaced by its fp32-rounded fp64 quotient."""
    return _with_g(c, lambda g: (g.double() / f32(scale)).float())


def aws_emul(c, hp, scale):
    return aw_emul(aws_quotient_case(c, scale), hp)


def aws_eval(c, hp, scale, outs, book=None, strict=True):
    """c holds the SCALED gradients; an accepted step (hp.found None or 0).  The fp64 reference with the fp64 quotient, and
    aw_eval's bounds plus the propagated rounding of the quotient (derivation in the module docstring)."""
    assert hp.found is None or hp.found == 0.0
    res = {}
    A = torch.abs

    def put(k, r):
        res[k] = max(res.get(k, 0.0), r)

    s = f32(scale)
    for T, o in zip(c.ts, outs):
        t = float(T.step) + 1.0 if T.step is not None else 1.0
        if T.step is not None:
            put("step", 0.0 if bits_equal(o.step, torch.tensor(t, dtype=F32)) else INF)
        p0, m0, v0 = T.p.double(), T.m.double(), T.v.double()
        q = T.g.double() / s
        d_g = E * A(q) + FLOOR
        m = hp.b1 * m0 + (1.0 - hp.b1) * q
        v = hp.b2 * v0 + (1.0 - hp.b2) * q * q
        x_m = (1.0 - hp.b1) * d_g
        x_v = (1.0 - hp.b2) * (2 * A(q) * d_g + d_g * d_g)
        bc1, bc2 = 1.0 - hp.b1 ** t, 1.0 - hp.b2 ** t
        sq = torch.sqrt(v) / math.sqrt(bc2)
        x_sq = torch.minimum(torch.where(v > 0, x_v / torch.sqrt(v).clamp_min(1e-300), torch.full_like(v, INF)), torch.sqrt(x_v)) / math.sqrt(bc2)
        den = sq + hp.eps
        ss = hp.lr / bc1
        upd = ss * m / den
        pw = p0 - hp.lr * hp.wd * p0
        p_ref = pw - upd
        d_den = 7 * E * sq + E * den + 2.0 ** -50
        d_upd = A(upd) * (6 * E + d_den / den) + ss * FLOOR / den + (ss * x_m + A(upd) * x_sq) / (den - x_sq).clamp_min(hp.eps)
        d_p = (E * A(pw) if hp.wd != 0.0 else 0.0) + d_upd + E * A(p_ref) + FLOOR
        dbl = 2.0 ** -50
        put("m", ratio(o.m, m, E * A(m) + dbl * (A(hp.b1 * m0) + A((1.0 - hp.b1) * q)) + FLOOR + x_m))
        put("v", ratio(o.v, v, (E + dbl) * A(v) + FLOOR + x_v))
        put("p", ratio(o.p, p_ref, d_p))
        if T.ema is None:
            assert o.ema is None
            continue
        e0 = T.ema.double()
        ew64 = 1.0 - hp.decay
        ew32 = f32(ew64)
        e_ref = e0 + ew64 * (p_ref - e0)
        d = A(p_ref - e0)
        tol = (ew32 * (d_p + E * d) + 2 * E * ew32 * d if ew32 < 0.5 else 2 * d_p + 3 * E * d) + E * A(e_ref) + FLOOR
        put("ema", ratio(o.ema, e_ref, tol))
    return judge("adamw_ema_scaled", F32, res, book, strict)


_AW = aw_case(seed=5)


def test_power_of_two_scaling_is_exact():
    hp = aw_hp(lr=1e-2, wd=0.01, decay=0.9)
    base = aw_emul(_AW, hp)
    for scale in POW2_SCALES:
        c2 = aws_pow2_case(_AW, scale)
        outs = aws_emul(c2, hp, scale)
        aw_eval(_AW, hp, outs, book={})
        assert all(bits_equal(getattr(o, k), getattr(b, k)) for o, b in zip(outs, base) for k in ("p", "m", "v"))
    with pytest.raises(AssertionError):
        aws_pow2_case(_AW, 2.0 ** 120)                                     # 1e4 * 2^120 overflows: the guard speaks


@pytest.mark.parametrize("scale", ODD_SCALES)
def test_scaled_emulation_meets_the_bound(scale, capsys):
    book = {}
    for hp in (aw_hp(), aw_hp(lr=1e-2, wd=0.01, decay=0.9), aw_hp(decay=0.25)):
        c2 = _with_g(_AW, lambda g: (g.double() * scale).float())          # what a scaled backward leaves: not exact
        aws_eval(c2, hp, scale, aws_emul(c2, hp, scale), book=book)
    with capsys.disabled():
        print(f"\nadamw with grad_scale {scale}: emulation error / bound {max(book.values()):.3f}")


def test_the_bound_notices_a_missing_unscale():
    hp = aw_hp(lr=1e-2, decay=0.9)
    c2 = _with_g(_AW, lambda g: (g.double() * 3.0).float())
    assert aws_eval(c2, hp, 3.0, aw_emul(c2, hp), strict=False) > 4.0        # never divided
