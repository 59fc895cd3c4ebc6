"""The fp16 loss scale on the device: dm_loss_scale_update against torch._amp_update_scale_ bit for bit, dm_adamw_ema_step with a
gradient scale against the existing fp64 bounds (power-of-two scales: exact) and the bound of tests/test_loss_scale_cpu.py (other
scales), and graphed.GraphedTrainStep with an optim.DeviceLossScale on a tiny denoiser: exactness against the unscaled step where
scaling is exact, and an overflow trajectory in which the host replays the update rule from the skips it observes.

The kernel cases go through the C ABI with hand-built structs inside sentinel frames, like tests/test_step_kernels_gpu.py, whose builders
they use.
"""
import copy
import itertools
import os
import socket
from types import SimpleNamespace as NS

import pytest
import torch

from tests.test_block_ops_gpu import _ok, _raw
from tests.test_loss_scale_cpu import ODD_SCALES, POW2_SCALES, _with_g, aws_eval, aws_pow2_case, f32, update_rule
from tests.test_mixer_passes_cpu import DM_ERR_ARG, EPS32, F32, FLOOR, bits_equal
from tests.test_step_kernels_cpu import aw_case, aw_eval, aw_hp
from tests.test_step_kernels_gpu import _aw_build, _aw_read, _chunk, _frame, _intact

pytestmark = pytest.mark.gpu

I32 = torch.int32


# =====================================================================================================================================
# dm_loss_scale_update
# =====================================================================================================================================
def _ls_args(scale, tracker, found, skipped, growth, backoff, interval):
    from diffma_amd._lib import dm_loss_scale_args

    a = dm_loss_scale_args()
    a.scale, a.growth_tracker, a.found_inf = scale.data_ptr(), tracker.data_ptr(), found.data_ptr()
    a.skipped = skipped.data_ptr() if skipped is not None else 0
    a.growth_factor, a.backoff_factor, a.growth_interval = growth, backoff, interval
    return a


def test_loss_scale_update_matches_torch_bit_for_bit(gpu):
    """found x tracker x interval x scale x factors, with and without `skipped`: every combination is one launch on its own element of
    a framed array next to one torch._amp_update_scale_ on a copy; one comparison at the end."""
    combos = []
    for interval in (1, 3, 2000):
        for found, tr, scale, (gf, bf) in itertools.product((0.0, 1.0), (0, interval - 2, interval - 1), (2.0 ** -120, 1.0, 65536.0, 3e38),
                                                            ((2.0, 0.5), (1.5, 0.3))):
            combos.append((f32(scale), tr, found, gf, bf, interval))
    n = len(combos)
    assert n == 144
    for with_skipped in (False, True):
        sc = _frame(gpu, F32, n, fill=torch.tensor([c[0] for c in combos], dtype=F32))
        tr = _frame(gpu, I32, n, fill=torch.tensor([c[1] for c in combos], dtype=I32))
        fo = _frame(gpu, F32, n, fill=torch.tensor([c[2] for c in combos], dtype=F32))
        sk = _frame(gpu, F32, n, fill=torch.arange(n, dtype=F32))
        rs, rt = sc.view.clone(), tr.view.clone()
        for i, (_, _, _, gf, bf, interval) in enumerate(combos):
            _ok("dm_loss_scale_update", _ls_args(sc.view[i:i + 1], tr.view[i:i + 1], fo.view[i:i + 1], sk.view[i:i + 1] if with_skipped else None,
                                                 gf, bf, interval))
            torch._amp_update_scale_(rs[i:i + 1], rt[i:i + 1], fo.view[i:i + 1], gf, bf, interval)
        torch.cuda.synchronize()
        for f, what in ((sc, "scale"), (tr, "tracker"), (fo, "found"), (sk, "skipped")):
            _intact(f, what)
        assert bits_equal(sc.view, rs) and bits_equal(tr.view, rt)
        host = [update_rule(*c) for c in combos]                     # ... and both are the rule of the CPU file
        assert [float(x) for x in sc.view.cpu()] == [h[0] for h in host] and tr.view.cpu().tolist() == [h[1] for h in host]
        big = [i for i, c in enumerate(combos) if c[0] > 1e38 and c[2] == 0.0 and c[1] == c[5] - 1]
        assert big and all(float(sc.view[i]) == combos[i][0] and int(tr.view[i]) == 0 for i in big), "3e38 must not grow"
        assert bits_equal(fo.view.cpu(), torch.tensor([c[2] for c in combos], dtype=F32))
        want = torch.arange(n, dtype=F32) + (torch.tensor([c[2] for c in combos], dtype=F32) if with_skipped else 0.0)
        assert bits_equal(sk.view.cpu(), want)


def test_loss_scale_update_sequence(gpu):
    """12 steps with a mixed found pattern on one (scale, tracker, skipped): torch, the kernel and the host rule agree after every step."""
    pattern = [0, 0, 1, 0, 0, 0, 1, 1, 0, 0, 0, 0]
    for gf, bf, interval, s0 in ((2.0, 0.5, 3, 65536.0), (1.5, 0.3, 2, 1.0), (2.0, 0.5, 1, f32(2.0e38))):
        sc, tr, sk = _frame(gpu, F32, 1, fill=torch.tensor([s0])), _frame(gpu, I32, 1, fill=torch.zeros(1, dtype=I32)), _frame(gpu, F32, 1, fill=torch.zeros(1))
        rs, rt = sc.view.clone(), tr.view.clone()
        hs, ht, seen = s0, 0, []
        for k, f in enumerate(pattern):
            found = torch.full((1,), float(f), device=gpu)
            _ok("dm_loss_scale_update", _ls_args(sc.view, tr.view, found, sk.view, gf, bf, interval))
            torch._amp_update_scale_(rs, rt, found, gf, bf, interval)
            hs, ht = update_rule(hs, ht, float(f), gf, bf, interval)
            seen.append((float(sc.view), int(tr.view), float(rs), int(rt), hs, ht))
        assert all(a == c == e and b == d == f for a, b, c, d, e, f in seen), seen
        assert float(sk.view) == float(sum(pattern))
        for f, what in ((sc, "scale"), (tr, "tracker"), (sk, "skipped")):
            _intact(f, what)


def test_loss_scale_update_status_codes_write_nothing(gpu):
    from diffma_amd import _lib

    inf, nan = float("inf"), float("nan")
    for kw in (dict(scale=0), dict(growth_tracker=0), dict(found_inf=0), dict(growth_interval=0), dict(growth_interval=-3), dict(growth_factor=0.0),
               dict(growth_factor=-2.0), dict(growth_factor=inf), dict(growth_factor=nan), dict(backoff_factor=0.0), dict(backoff_factor=-0.5),
               dict(backoff_factor=inf), dict(backoff_factor=nan)):
        fr = [_frame(gpu, F32, 1, fill=torch.tensor([65536.0])), _frame(gpu, I32, 1, fill=torch.tensor([2], dtype=I32)),
              _frame(gpu, F32, 1, fill=torch.tensor([1.0])), _frame(gpu, F32, 1, fill=torch.tensor([5.0]))]
        before = [f.buf.clone() for f in fr]
        a = _ls_args(fr[0].view, fr[1].view, fr[2].view, fr[3].view, 2.0, 0.5, 3)
        for k, v in kw.items():
            setattr(a, k, v)
        assert _raw("dm_loss_scale_update", a) == DM_ERR_ARG, kw
        torch.cuda.synchronize()
        assert all(bits_equal(x, f.buf) for x, f in zip(before, fr)), kw
    assert int(_lib.load().dm_loss_scale_update(None, None)) == DM_ERR_ARG


def test_loss_scale_update_is_capturable(gpu):
    """Replayed from a hipGraph through optim.DeviceLossScale: three replays with found = 0, 0, 1 at interval 2."""
    from diffma_amd import optim

    ls = optim.DeviceLossScale(gpu, init_scale=8.0, growth_interval=2)
    found, skipped = torch.zeros((), device=gpu), torch.zeros((), device=gpu)
    side = torch.cuda.Stream(device=gpu)
    side.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(side):
        ls.update(found)
    torch.cuda.current_stream(gpu).wait_stream(side)
    ls.load_state_dict(dict(ls.state_dict(), scale=8.0, _growth_tracker=0))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ls.update(found, skipped=skipped)
    assert ls.state_dict()["scale"] == 8.0 and ls.state_dict()["_growth_tracker"] == 0        # a capture runs nothing
    seen = []
    for f in (0.0, 0.0, 1.0):
        found.fill_(f)
        graph.replay()
        seen.append((float(ls.scale), int(ls.growth_tracker), float(skipped)))
    assert seen == [(8.0, 1, 0.0), (16.0, 0, 0.0), (8.0, 0, 1.0)], seen


# =====================================================================================================================================
# dm_adamw_ema_step with grad_scale
# =====================================================================================================================================
def _aw_case():
    return aw_case(seed=5, chunk=_chunk())


def _aws_run(gpu, c_dev, hp, scale, **kw):
    """One call on case c_dev (whose gradients are what the device holds) with grad_scale -> `scale` (None: NULL)."""
    m = _aw_build(gpu, c_dev, hp, **kw)
    if scale is not None:
        m.scale = _frame(gpu, F32, 1, fill=torch.tensor([scale], dtype=F32))
        m.a.grad_scale = m.scale.view.data_ptr()
    _ok("dm_adamw_ema_step", m.a)
    outs = _aw_read(m)
    if scale is not None:
        _intact(m.scale, "grad_scale")
        assert float(m.scale.view) == f32(scale), "the scale is read-only"
    for T, fr in zip(c_dev.ts, m.fr):                                # the unscaled gradient is not written back
        if not kw.get("g_nan"):
            assert bits_equal(fr["g"].view, T.g)
    return outs


def _same(a, b):
    return all(bits_equal(getattr(x, k), getattr(y, k)) for x, y in zip(a, b) for k in ("p", "m", "v", "ema", "step") if getattr(x, k) is not None)


def test_adamw_power_of_two_scales_are_exact(gpu):
    """The device gradient is g * scale (exact, asserted); the outputs pass the EXISTING bound of the unscaled case, agree bit for bit
    with the grad_scale = NULL run of the unscaled case, in the 16-byte arm and (g one element off a boundary) the element-wise arm."""
    c = _aw_case()
    for hp in (aw_hp(), aw_hp(lr=1e-2, wd=0.01, decay=0.9), aw_hp(found=0.0, decay=0.25)):
        for mis in (None, "g"):
            base = _aws_run(gpu, c, hp, None, mis=mis)
            aw_eval(c, hp, base)
            for scale in POW2_SCALES:
                outs = _aws_run(gpu, aws_pow2_case(c, scale), hp, scale, mis=mis)
                aw_eval(c, hp, outs)
                assert _same(outs, base), (scale, mis)


@pytest.mark.parametrize("scale", ODD_SCALES)
def test_adamw_other_scales_within_the_propagated_bound(gpu, scale, capsys):
    c = _with_g(_aw_case(), lambda g: (g.double() * scale).float())
    book = {}
    for hp in (aw_hp(), aw_hp(lr=1e-2, wd=0.01, decay=0.9)):
        for mis in (None, "g", "p"):
            aws_eval(c, hp, scale, _aws_run(gpu, c, hp, scale, mis=mis), book=book)
    with capsys.disabled():
        print(f"\nadamw with grad_scale {scale}: error / bound {max(book.values()):.3f}")


def test_adamw_skipped_step_with_a_scale(gpu):
    """found_inf = 1, NaN gradients and a scale set: p, m, v and the counters bit-unchanged (aw_eval's skip arm), the EMA moves with
    ema_on_skip and stays without."""
    c = _aw_case()
    for on in (0, 1):
        hp = aw_hp(decay=0.9, found=1.0, ema_on_skip=on)
        outs = _aws_run(gpu, c, hp, 65536.0, g_nan=True)
        aw_eval(c, hp, outs)
        for o, T in zip(outs, c.ts):
            assert bits_equal(o.p, T.p) and bits_equal(o.m, T.m) and bits_equal(o.v, T.v)
            assert T.step is None or bits_equal(o.step, T.step)
        assert any(not bits_equal(o.ema, T.ema) for o, T in zip(outs, c.ts) if T.ema is not None) == bool(on)


def test_fused_wrapper_passes_the_scale(gpu):
    from diffma_amd import optim

    g = torch.Generator().manual_seed(3)
    p0, gr = torch.randn(4099, generator=g), torch.randn(4099, generator=g)
    res = []
    for scale in (None, 1024.0):
        p = torch.nn.Parameter(p0.clone().to(gpu))
        opt = torch.optim.AdamW([p], lr=1e-2, weight_decay=0.0)
        fused = optim.FusedAdamWEMA(opt, [p])
        p.grad = (gr * (scale or 1.0)).to(gpu)
        fused.step(grad_scale=None if scale is None else torch.full((), scale, device=gpu))
        res.append((p.detach().cpu(), opt.state[p]["exp_avg"].cpu(), opt.state[p]["exp_avg_sq"].cpu()))
    assert all(bits_equal(a, b) for a, b in zip(*res)) and not bits_equal(res[0][0], p0)


# =====================================================================================================================================
# graphed.GraphedTrainStep with a DeviceLossScale
# =====================================================================================================================================
_TINY = {}
_RUNS = {}


def _tiny(gpu):
    if not _TINY:
        from diffma_amd.diffusion import create_diffusion
        from diffma_amd.model import DiffMa

        torch.manual_seed(21)
        net0 = DiffMa(input_size=8, patch_size=2, strip_size=2, hidden_size=64, depth=2, d_state=16).to(gpu)
        with torch.no_grad():
            for p in net0.parameters():
                if float(p.abs().max()) == 0.0:
                    p.normal_(0, 0.02)
        B = 4
        mk = lambda *sh: torch.randn(*sh, device=gpu)
        _TINY.update(net0=net0, B=B, x=mk(B, 4, 8, 8), y=mk(B, 64), y2=mk(B, 16, 64), w=torch.sigmoid(mk(B, 16, 1)),
                     t=torch.tensor([3, 250, 600, 999], device=gpu), d=create_diffusion(""))
    return NS(**_TINY)


def _state(net, ema, opt):
    st = [opt.state[p] for p in net.parameters() if p in opt.state]
    return NS(p=[p.detach().clone() for p in net.parameters()], e=[p.detach().clone() for p in ema.parameters()],
              m=[s["exp_avg"].clone() for s in st], v=[s["exp_avg_sq"].clone() for s in st], step=[s["step"].clone() for s in st])


def _run(gpu, steps, amp=None, ls=None, split=False, stages=None, watch=False, seed=11):
    """`steps` graphed steps on the fixed batch.  ls: keyword arguments of DeviceLossScale (None: no loss scale).  watch: after every
    step read skipped, scale and tracker, and keep the state before and after."""
    from diffma_amd import optim
    from diffma_amd.graphed import GraphedTrainStep

    T = _tiny(gpu)
    torch.manual_seed(seed)
    net = copy.deepcopy(T.net0).train()
    ema = copy.deepcopy(net).requires_grad_(False)
    opt = torch.optim.AdamW(net.parameters(), lr=1e-3, weight_decay=0, fused=True, capturable=True)
    scale = optim.DeviceLossScale(gpu, **ls) if ls is not None else None
    kw = {} if scale is None else dict(loss_scale=scale)
    gs = GraphedTrainStep(net, ema, opt, T.d, T.x, T.t, T.y, T.y2, T.w, autocast_dtype=amp, ema_decay=0.9, warmup=2, split=split, stages=stages, **kw)
    assert gs.split == split and float(gs.skipped) == 0.0
    if scale is not None:                                            # construction leaves the scale as it found it
        assert float(scale.scale) == f32(ls.get("init_scale", 65536.0)) and int(scale.growth_tracker) == 0
    r = NS(losses=[], skipped=[], scale=[], tracker=[], before=[], after=[], gs=gs, ls=scale)
    for _ in range(steps):
        if watch:
            r.before.append(_state(net, ema, opt))
        r.losses.append(float(gs.step(T.x, T.t, T.y, T.y2, T.w)))
        r.skipped.append(float(gs.skipped))
        if scale is not None:
            r.scale.append(float(scale.scale))
            r.tracker.append(int(scale.growth_tracker))
        if watch:
            r.after.append(_state(net, ema, opt))
    r.final = _state(net, ema, opt)
    return r


def _equal_states(a, b, names=("p", "e", "m", "v", "step")):
    return all(len(getattr(a, k)) == len(getattr(b, k)) and all(torch.equal(x, y) for x, y in zip(getattr(a, k), getattr(b, k))) for k in names)


def test_graphed_fp32_fixed_power_of_two_scale_is_exact(gpu, capsys):
    """Scaling a linear backward by 2^10 is exact in fp32: losses, weights, EMA and exp_avg_sq equal the unscaled run's; exp_avg may
    differ only below 2^-100 (fp32-subnormal gradients that the scale rescues)."""
    a = _run(gpu, 4)
    b = _run(gpu, 4, ls=dict(init_scale=2.0 ** 10, growth_interval=10 ** 9))
    assert a.skipped[-1] == 0.0 and b.skipped[-1] == 0.0 and b.scale == [1024.0] * 4 and b.tracker == [1, 2, 3, 4]
    assert all(l == l for l in a.losses) and a.losses == b.losses, (a.losses, b.losses)
    assert _equal_states(a.final, b.final, ("p", "e", "v", "step"))
    rescued = 0
    for x, y in zip(a.final.m, b.final.m):
        diff = x != y
        rescued += int(diff.sum())
        assert bool(((x.abs() < FLOOR) & (y.abs() < FLOOR))[diff].all())
    with capsys.disabled():
        print(f"\nexp_avg elements that differ below 2^-100: {rescued}")


def test_graphed_fp16_scale_one_equals_no_scale(gpu):
    a = _run(gpu, 4, amp=torch.float16)
    b = _run(gpu, 4, amp=torch.float16, ls=dict(init_scale=1.0, growth_interval=10 ** 9))
    assert a.losses == b.losses and a.skipped == b.skipped and b.scale == [1.0] * 4
    assert _equal_states(a.final, b.final)


TRAJ = dict(init_scale=2.0 ** 30, growth_interval=3)
TRAJ_STEPS = 40


def _unscaled_fp16(gpu):
    if "plain" not in _RUNS:
        _RUNS["plain"] = _run(gpu, TRAJ_STEPS, amp=torch.float16)
    return _RUNS["plain"]


def _check_trajectory(gpu, r, decay=0.9):
    """The host replays the rule of the CPU file from the skips it observes and demands the exact scale and tracker; a skipped step
    leaves weights, moments and counters bit-unchanged and moves the EMA by 0.9 e + 0.1 p (within the fp32 roundings of
    e + w (p - e): w = (float)0.1, the difference, the product, the sum -- 3 E w |p - e| + E |result| + 2^-100)."""
    s, t, prev = TRAJ["init_scale"], 0, 0.0
    found, grown = [], 0
    for k in range(TRAJ_STEPS):
        f = r.skipped[k] - prev
        prev = r.skipped[k]
        assert f in (0.0, 1.0), (k, r.skipped)
        found.append(f)
        s2, t = update_rule(s, t, f, interval=TRAJ["growth_interval"])
        grown += s2 > s
        s = s2
        assert (r.scale[k], r.tracker[k]) == (s, t), (k, found, r.scale, r.tracker)
        b, a = r.before[k], r.after[k]
        if f:
            assert _equal_states(a, b, ("p", "m", "v", "step")), k
            for e0, e1, p in zip(b.e, a.e, b.p):
                ref = 0.9 * e0.double() + 0.1 * p.double()
                tol = 3 * EPS32 * 0.1 * (p.double() - e0.double()).abs() + EPS32 * ref.abs() + FLOOR
                assert bool(((e1.double() - ref).abs() <= tol).all()), k
        else:
            assert not _equal_states(a, b, ("p",)) and all(float(x) == float(y) + 1.0 for x, y in zip(a.step, b.step)), k
            assert all(bool(torch.isfinite(x).all()) for x in a.p + a.m + a.v), k
    assert sum(found) >= 1 and sum(found) < TRAJ_STEPS and grown >= 1, (found, r.scale)
    return found


def test_graphed_fp16_overflow_trajectory(gpu, capsys):
    plain = _unscaled_fp16(gpu)
    assert plain.skipped[-1] == 0.0 and all(l == l for l in plain.losses), "precondition: the unscaled fp16 run skips nothing"
    r = _run(gpu, TRAJ_STEPS, amp=torch.float16, ls=TRAJ, watch=True)
    found = _check_trajectory(gpu, r)
    _RUNS["traj"] = r
    again = _run(gpu, TRAJ_STEPS, amp=torch.float16, ls=TRAJ)
    same = lambda x, y: len(x) == len(y) and all(a == b or (a != a and b != b) for a, b in zip(x, y))
    assert same(r.losses, again.losses) and r.skipped == again.skipped and r.scale == again.scale
    with capsys.disabled():
        print(f"\nfound: {''.join(str(int(f)) for f in found)}  scale: 2^30 -> {r.scale[-1]:g}")


def _dist_env(monkeypatch):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    for k, v in dict(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0").items():
        monkeypatch.setenv(k, v)


def _one_rank_group(gpu, monkeypatch):
    import torch.distributed as dist

    if not dist.is_initialized():
        _dist_env(monkeypatch)
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=gpu)


def test_graphed_fp16_two_graphs_equal_one_graph(gpu, monkeypatch):
    _one_rank_group(gpu, monkeypatch)
    one = _run(gpu, 8, amp=torch.float16, ls=TRAJ)
    two = _run(gpu, 8, amp=torch.float16, ls=TRAJ, split=True)
    assert one.skipped[-1] >= 1.0, "the case must contain a skipped step"
    for a, b in zip(one.losses, two.losses):
        assert a == b or (a != a and b != b), (one.losses, two.losses)
    assert one.skipped == two.skipped and one.scale == two.scale and one.tracker == two.tracker
    for a, b in zip(one.final.p + one.final.e, two.final.p + two.final.e):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_graphed_fp16_trajectory_with_torchs_optimiser(gpu, monkeypatch):
    """DIFFMA_FUSED_OPT=0: torch's unscale + fused AdamW + lerp in the graph, the same device-side scale update."""
    from diffma_amd import optim

    monkeypatch.setattr(optim, "ENABLED", False)
    plain = _unscaled_fp16(gpu)
    assert plain.skipped[-1] == 0.0, "precondition: the unscaled fp16 run skips nothing"
    r = _run(gpu, TRAJ_STEPS, amp=torch.float16, ls=TRAJ, watch=True)
    assert r.gs._fused is None
    _check_trajectory(gpu, r)


def test_graphed_fp16_two_graphs_equal_one_graph_with_torchs_optimiser(gpu, monkeypatch):
    """DIFFMA_FUSED_OPT=0 in the two-graph form: the gradients come back from the flat buffer scaled and go through the same unscale as
    in the one-graph form; 8 steps of the overflow trajectory, everything equal."""
    import torch.distributed as dist

    from diffma_amd import optim

    monkeypatch.setattr(optim, "ENABLED", False)
    _one_rank_group(gpu, monkeypatch)
    one = _run(gpu, 8, amp=torch.float16, ls=TRAJ)
    two = _run(gpu, 8, amp=torch.float16, ls=TRAJ, split=True)
    assert one.gs._fused is None and two.gs._fused is None and dist.is_initialized()
    assert one.skipped[-1] >= 1.0, "the case must contain a skipped step"
    for a, b in zip(one.losses, two.losses):
        assert a == b or (a != a and b != b), (one.losses, two.losses)
    assert one.skipped == two.skipped and one.scale == two.scale and one.tracker == two.tracker
    for a, b in zip(one.final.p + one.final.e, two.final.p + two.final.e):
        torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_staged_form_refuses_a_loss_scale(gpu):
    with pytest.raises(ValueError):
        _run(gpu, 1, amp=torch.float16, ls=TRAJ, stages=4)


@pytest.mark.parametrize("flag", ["1", "0"])
def test_scale_seed_passes_through_the_loss(gpu, monkeypatch, flag):
    """A 0-dim fp32 seed through loss.mean() and the loss backward (fused kernel and the generic expression): the gradients are the
    unseeded ones times the seed, exactly for a power of two (DIFFMA_FUSED_LOSS = 1 and 0)."""
    T = _tiny(gpu)
    monkeypatch.setattr(T.d, "fused_loss", flag == "1", raising=False)          # what DIFFMA_FUSED_LOSS sets when the class is defined
    grads = []
    for seed in (None, torch.full((), 256.0, device=gpu)):
        net = copy.deepcopy(T.net0).train()
        torch.manual_seed(2)
        loss = T.d.training_losses(net, T.x, T.t, dict(y=T.y, y2=T.y2, w=T.w))["loss"].mean()
        assert loss.dtype == F32 and loss.dim() == 0
        loss.backward() if seed is None else loss.backward(gradient=seed)
        grads.append([p.grad.clone() for p in net.parameters() if p.grad is not None])
    assert len(grads[0]) == len(grads[1]) > 0
    for a, b in zip(*grads):
        diff = a * 256.0 != b
        assert bool((b[diff].abs() < 256.0 * FLOOR).all()), "only a gradient in fp32's denormal range may differ"


@pytest.fixture
def gemm_tuning_restored():
    """train.main switches PyTorch's TunableOp on for the whole process (recorded table + online tuning of unseen shapes); tests that
    run later in the same process must not inherit online tuning (tests/test_drivers_gpu.py isolates its driver tests the same way)."""
    yield
    import torch.cuda.tunable as tunable

    tunable.tuning_enable(False)
    tunable.enable(False)


def test_train_main_fp16_graphed(gpu, monkeypatch, tmp_path, gemm_tuning_restored):
    """train.main in the reference's own mode (fp16 autocast, loss scale) with the graphed step: three counted steps, one checkpoint
    in the reference's format with finite weights, and a step count that is the number of replays minus the skipped ones."""
    from diffma_amd import graphed as graphed_mod
    from diffma_amd import train as train_mod
    from diffma_amd.config import Config

    _dist_env(monkeypatch)
    seen = NS(calls=0, skipped=0.0, with_scale=[])
    real = graphed_mod.GraphedTrainStep.step

    def step(self, *a, **k):                                         # counts the replays; keeps numbers, not the object
        out = real(self, *a, **k)
        seen.calls += 1
        seen.skipped = float(self.skipped)
        seen.with_scale.append(self.ls is not None and self.amp == torch.float16)
        return out

    monkeypatch.setattr(graphed_mod.GraphedTrainStep, "step", step)
    cfg = Config(model="DiffMa-S/2", image_size=224, dt_rank=16, d_state=16, global_batch_size=4, global_seed=0, lr=1e-4, lr_=1e-4,
                 epochs=1, accumulation_steps=1, log_every=1, ckpt_every=3, results_dir=str(tmp_path / "res"),
                 init_from_pretrain_ckpt=False, pretrain_ckpt_path="", init_train_steps=0, synthetic=True, synthetic_samples=64,
                 max_steps=3, autocast=True, amp_dtype="fp16", graph_train=True, grad_compression="none", use_mamba2=False)
    steps = train_mod.main(cfg)
    assert steps == 3 and seen.calls >= 3 and all(seen.with_scale)
    assert steps == seen.calls - int(seen.skipped)
    ck = [os.path.join(dp, f) for dp, _, fs in os.walk(tmp_path) for f in fs if f.endswith(".pt")]
    assert len(ck) == 1 and ck[0].endswith("0000003.pt"), ck
    sd = torch.load(ck[0], map_location="cpu", weights_only=False)
    assert set(sd) == {"model", "ema", "opt", "args"}
    assert all(torch.isfinite(v).all() for v in sd["model"].values()) and all(torch.isfinite(v).all() for v in sd["ema"].values())
