"""csrc/diffusion_loss.hip, csrc/diffusion_step.hip and csrc/optim.hip operator by operator against fp64: dm_q_sample, dm_training_loss,
dm_training_loss_bwd, dm_diffusion_step, dm_adamw_ema_step and dm_grads_nonfinite.

The calls go through the C ABI with hand-built structs, so the shapes, the table layout (permuted rows with NaN rows between them), the
block order, the alignment of every pointer and every NULL are chosen by the test rather than by the wrappers.  Builders, fp64
references and bound functions -- with their derivations -- are in tests/test_step_kernels_cpu.py; the kernels' outputs go through the
same `*_eval` functions as the emulations there.  Every output is a NaN-filled view inside a sentinel frame that is compared afterwards.

Largest error-to-bound ratio on the MI355X when this file was written (test_zz_error_to_bound_ratios prints them under -s):
    q_sample          fp32 0.977                            training_loss_bwd fp32 1.000  bf16 0.996  fp16 0.998
    training_loss     fp32 0.952  bf16 0.967  fp16 0.978    diffusion_step    fp32 0.965  bf16 0.958  fp16 0.962
    adamw_ema         fp32 1.000                            grads_nonfinite   exact
(measured against the fp64 reference, not targets.  AdamW with p, m, v, g or ema one element off a 16-byte boundary came out
bit-identical to the all-aligned run in all five classes.)
"""
from types import SimpleNamespace as NS

import pytest
import torch

from tests.test_block_ops_gpu import _ok, _raw
from tests.test_mixer_passes_cpu import CODE, DM_ERR_ARG, DTYPES, F32, NAME, NAN, bits_equal
from tests.test_step_kernels_cpu import (BAD_T, GRID, INF, LOSS_ROWS, RATIOS, STEP_ROWS, aw_case, aw_eval, aw_hp, aw_hps, ds_big,
                                         ds_case, ds_cases, ds_eval, lb_cases, lb_eval, nf_case, nf_eval, nf_positions, qs_case, qs_cases,
                                         qs_eval, schedule, tl_big, tl_case, tl_cases, tl_eval)

pytestmark = pytest.mark.gpu

SENT = 7.0
IDS = list(NAME.values())
LOSS_FIELDS = ("row_sqrt_ac", "row_sqrt_1mac", "row_post_logvar", "row_log_betas", "row_sqrt_recip_ac", "row_sqrt_recipm1_ac", "row_coef1",
               "row_coef2")
STEP_FIELDS = ("row_post_logvar", "row_log_betas", "row_sqrt_recip_ac", "row_sqrt_recipm1_ac", "row_coef1", "row_coef2", "row_ac",
               "row_ac_prev")
_TAB = {}


def _frame(gpu, dt, n, off=8, fill=None):
    """n elements starting `off` elements into a sentinel-filled buffer; NaN in the view unless `fill` is given."""
    buf = torch.full((off + n + 16,), SENT, dtype=dt, device=gpu)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + n]
    if fill is None:
        view.fill_(NAN)
    else:
        view.copy_(fill.reshape(-1))
    return NS(buf=buf, view=view, off=off, n=n)


def _intact(f, what):
    assert bool((f.buf[:f.off] == SENT).all()) and bool((f.buf[f.off + f.n:] == SENT).all()), f"{what}: the kernel wrote outside its view"


def _untouched(f):
    return bool(f.view.isnan().all())


def _tables(gpu, s):
    if s.spec not in _TAB:
        _TAB[s.spec] = s.tab.to(gpu)
    return _TAB[s.spec]


def _bad_t(T):
    return [T if b is None else b for b in BAD_T]


# =====================================================================================================================================
# dm_q_sample / dm_training_loss / dm_training_loss_bwd
# =====================================================================================================================================
def _loss_struct(gpu, c, dt, keep):
    from diffma_amd._lib import dm_training_loss_args

    a = dm_training_loss_args()
    a.batch, a.channels, a.hw, a.T, a.out_dtype = c.B, c.C, c.hw, c.s.T, CODE[dt]
    for f, k in zip(LOSS_FIELDS, LOSS_ROWS):
        setattr(a, f, c.s.row[k])
    t = c.t.to(gpu)
    keep.append(t)
    a.t, a.tables = t.data_ptr(), _tables(gpu, c.s).data_ptr()
    return a


def _dev(gpu, keep, *xs):
    out = [x.contiguous().to(gpu) for x in xs]
    keep += out
    return [x.data_ptr() for x in out]


def _qs_run(gpu, c):
    keep = []
    a = _loss_struct(gpu, c, F32, keep)
    a.x_start, a.noise = _dev(gpu, keep, c.x0, c.nz)
    out = _frame(gpu, F32, c.B * c.per)
    a.x_t_out = out.view.data_ptr()
    _ok("dm_q_sample", a)
    torch.cuda.synchronize()
    _intact(out, "q_sample x_t")
    got = out.view.cpu().view(c.B, c.per)
    qs_eval(c, got)
    return got


def test_q_sample_shapes_and_every_timestep(gpu):
    """batch 5, C 3, hw 7 with mixed t (0, 1, T - 1 among them) and every timestep of both schedules at batch T, C 1, hw 8."""
    for c in qs_cases()[:-1]:
        _qs_run(gpu, c)


def test_q_sample_second_grid_stride_trip(gpu):
    """batch 3, C 1, hw 350 003 = 1 050 009 elements: the last 1433 take the second trip; per is odd, three different t."""
    c = qs_cases()[-1]
    assert c.B * c.per > GRID and c.per % 2 == 1 and len(set(c.t.tolist())) == 3
    _qs_run(gpu, c)


def _tl_run(gpu, c):
    keep = []
    a = _loss_struct(gpu, c, c.dt, keep)
    a.model_out, a.x_start, a.x_t, a.noise = _dev(gpu, keep, c.mo, c.x0, c.xt, c.nz)
    fr = NS(mse=_frame(gpu, F32, c.B), vb=_frame(gpu, F32, c.B), loss=_frame(gpu, F32, c.B), grad=_frame(gpu, F32, c.B * 2 * c.per))
    a.mse, a.vb, a.loss, a.grad = (f.view.data_ptr() for f in (fr.mse, fr.vb, fr.loss, fr.grad))
    _ok("dm_training_loss", a)
    torch.cuda.synchronize()
    for k, f in vars(fr).items():
        _intact(f, "training_loss " + k)
    mse, vb, loss, grad = fr.mse.view.cpu(), fr.vb.view.cpu(), fr.loss.view.cpu(), fr.grad.view.cpu().view(c.B, 2 * c.per)
    tl_eval(c, mse, vb, loss, grad)
    return mse, vb, loss, grad


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_training_loss_per_classes_and_every_timestep(gpu, dt):
    """per 1, 63, 255, 256, 257, 3136 at batch 1 and 7, every timestep of both schedules at C 1, hw 8, and the t = 0 decoder construction
    at per 3136 (an all-live, an all-dead and a mixed sample, all three branches): mse, vb, loss and both halves of grad within bound of
    fp64, loss == mse + vb bit for bit, the v-gradient of every clamped element exactly 0."""
    for c in tl_cases(dt, big=False):
        _tl_run(gpu, c)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_training_loss_long_per_thread_chain(gpu, dt):
    """per = 175 003: 684 additions per thread in the sample sums, one t = 0 sample and one KL sample."""
    c = tl_big(dt)
    assert -(-c.per // 256) == 684
    _tl_run(gpu, c)


def _lb_run(gpu, c):
    from diffma_amd._lib import dm_training_loss_args

    keep = []
    a = dm_training_loss_args()
    a.batch, a.channels, a.hw, a.T, a.out_dtype = c.B, c.C, c.hw, 1, CODE[c.dt]
    a.grad, a.g_eps, a.g_v = _dev(gpu, keep, c.grad, c.g_eps, c.g_v)
    out = _frame(gpu, c.dt, c.B * 2 * c.per)
    a.grad_out = out.view.data_ptr()
    _ok("dm_training_loss_bwd", a)
    torch.cuda.synchronize()
    _intact(out, "training_loss_bwd grad_out")
    lb_eval(c, out.view.cpu().view(c.B, 2 * c.per))


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_training_loss_bwd_small_and_second_trip(gpu, dt):
    """batch 5, C 3, hw 7 and batch 3, C 1, hw 175 003 (1 050 018 elements, second trip); g_eps and g_v distinct per sample with 0 and
    negative values among them."""
    small, big = lb_cases(dt)
    assert big.B * 2 * big.per > GRID
    for c in (small, big):
        assert len(set(c.g_eps.tolist())) == c.B and len(set(c.g_v.tolist())) == c.B
        assert 0.0 in c.g_eps.tolist() and 0.0 in c.g_v.tolist() and min(c.g_v.tolist()) < 0
        _lb_run(gpu, c)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_out_of_range_timesteps_poison_their_sample_only(gpu, dt):
    """t in {-1, T, 2^40} between valid samples: x_t, mse, vb, loss and both halves of grad of those samples are NaN, the others stay
    within bound (the evaluation demands NaN exactly where the reference has it)."""
    for spec in ("", "250"):
        T = schedule(spec).T
        bad = _bad_t(T)
        t = [3, bad[0], T - 1, bad[1], 0, bad[2], 7]
        if dt == F32:
            got = _qs_run(gpu, qs_case(spec, 7, 3, 7, t=t, seed=70))
            assert bool(got[[1, 3, 5]].isnan().all()) and bool(got[[0, 2, 4, 6]].isfinite().all())
        mse, vb, loss, grad = _tl_run(gpu, tl_case(dt, spec, 7, 3, 7, t=t, seed=71))
        for x in (mse, vb, loss, grad):
            assert bool(x[[1, 3, 5]].isnan().all()) and bool(x[[0, 2, 4, 6]].isfinite().all())


# =====================================================================================================================================
# dm_diffusion_step
# =====================================================================================================================================
def _ds_run(gpu, c, pred=True):
    from diffma_amd._lib import dm_diffusion_step_args

    keep = []
    a = dm_diffusion_step_args()
    a.batch, a.channels, a.hw, a.T, a.mode, a.clip, a.out_dtype, a.eta = c.B, c.C, c.hw, c.s.T, c.mode, c.clip, CODE[c.dt], c.eta
    for f, k in zip(STEP_FIELDS, STEP_ROWS):
        setattr(a, f, c.s.row[k])
    a.model_out, a.x, a.t = _dev(gpu, keep, c.mo, c.x, c.t)
    if c.nz is not None:
        (a.noise,) = _dev(gpu, keep, c.nz)
    a.tables = _tables(gpu, c.s).data_ptr()
    smp, x0 = _frame(gpu, F32, c.B * c.per), _frame(gpu, F32, c.B * c.per)
    a.sample = smp.view.data_ptr()
    if pred:
        a.pred_xstart = x0.view.data_ptr()
    _ok("dm_diffusion_step", a)
    torch.cuda.synchronize()
    _intact(smp, "diffusion_step sample")
    _intact(x0, "diffusion_step pred_xstart")
    if not pred:
        assert _untouched(x0), "pred_xstart == NULL: its would-be buffer was written"
    s, p = smp.view.cpu().view(c.B, c.per), (x0.view.cpu().view(c.B, c.per) if pred else None)
    ds_eval(c, s, p)
    return s, p


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_diffusion_step_modes_clip_and_every_timestep(gpu, dt):
    """DDPM, and DDIM with eta 0, 0.5 and 1; clip off and on with x0 leaving [-1, 1] on both sides; every timestep of both schedules
    at batch T, C 1, hw 8 and mixed t at batch 5, C 3, hw 7: sample and pred_xstart within bound of fp64, every sample finite."""
    for c in ds_cases(dt, big=False):
        _ds_run(gpu, c)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_diffusion_step_second_grid_stride_trip(gpu, dt):
    """batch 3, C 1, hw 350 003: the last 1433 elements take the second trip, t = 0, 3, 999."""
    for c in ds_big(dt):
        assert c.B * c.per > GRID
        _ds_run(gpu, c)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_diffusion_step_null_noise_null_pred_and_t0(gpu, dt):
    """noise == NULL (no noise term); pred_xstart == NULL (its frame untouched, the sample unchanged bit for bit); at t = 0 the noise
    is masked, so a sample with t = 0 is bit-equal with and without a noise pointer."""
    for mode, eta in ((0, 0.0), (1, 1.0)):
        kw = dict(t=[0, 5, 0, 200, 999], seed=80 + mode)
        with_nz = ds_case(dt, "", 5, 3, 7, mode, eta, 1, **kw)
        no_nz = ds_case(dt, "", 5, 3, 7, mode, eta, 1, noise=False, **kw)
        s1, p1 = _ds_run(gpu, with_nz)
        s0, p0 = _ds_run(gpu, no_nz)
        s2, _ = _ds_run(gpu, with_nz, pred=False)
        assert bits_equal(s1[[0, 2]], s0[[0, 2]]) and not bits_equal(s1[[1, 3, 4]], s0[[1, 3, 4]])
        assert bits_equal(p1, p0) and bits_equal(s2, s1)


@pytest.mark.parametrize("dt", DTYPES, ids=IDS)
def test_diffusion_step_out_of_range_timestep_is_nan(gpu, dt):
    """The guard of diffusion_step_kernel: t in {-1, T, 2^40} reads no table entry; that sample's sample and pred_xstart are NaN, the
    others stay within bound."""
    for spec in ("", "250"):
        T = schedule(spec).T
        bad = _bad_t(T)
        for mode, eta in ((0, 0.0), (1, 0.5)):
            c = ds_case(dt, spec, 7, 3, 7, mode, eta, 1, t=[3, bad[0], T - 1, bad[1], 0, bad[2], 7], seed=90 + mode)
            s, p = _ds_run(gpu, c)
            for x in (s, p):
                assert bool(x[[1, 3, 5]].isnan().all()) and bool(x[[0, 2, 4, 6]].isfinite().all())
            _ds_run(gpu, c, pred=False)


# =====================================================================================================================================
# dm_adamw_ema_step
# =====================================================================================================================================
AW_NAMES = ("p", "m", "v", "g", "ema")


def _chunk():
    from diffma_amd import _lib

    return int(_lib.load().dm_adamw_chunk())


def _aw_build(gpu, c, hp, mis=None, g_nan=False, only_g=False):
    """The table, the block arrays and the args struct of case c.  `mis` names the one pointer of every row that sits one element off a
    16-byte boundary.  only_g: the rows dm_grads_nonfinite reads (g and n), every other pointer NULL."""
    from diffma_amd._lib import dm_adamw_args

    m = NS(c=c, hp=hp, fr=[], keep=[])
    nt = len(c.ts)
    m.steps = _frame(gpu, F32, nt)
    rows = []
    for i, T in enumerate(c.ts):
        fr = {}
        for k in (("g",) if only_g else AW_NAMES):
            src = getattr(T, k)
            if src is None:
                fr[k] = None
                continue
            fr[k] = _frame(gpu, F32, T.n, off=8 + (mis == k), fill=torch.full_like(src, NAN) if (k == "g" and g_nan) else src)
            assert (fr[k].view.data_ptr() % 16 == 0) == (mis != k)
        if not only_g and T.step is not None:
            m.steps.view[i] = float(T.step)
        m.fr.append(fr)
        ptr = lambda k: fr[k].view.data_ptr() if fr.get(k) is not None else 0
        rows.append([ptr("p"), ptr("m"), ptr("v"), ptr("g"), ptr("ema"),
                     m.steps.view.data_ptr() + 4 * i if (not only_g and T.step is not None) else 0, T.n])
    m.table = torch.tensor(rows, dtype=torch.int64).to(gpu)
    m.bt, m.bc = torch.tensor(c.bt, dtype=torch.int32).to(gpu), torch.tensor(c.bc, dtype=torch.int32).to(gpu)
    a = dm_adamw_args()
    a.tensors, a.block_tensor, a.block_chunk = m.table.data_ptr(), m.bt.data_ptr(), m.bc.data_ptr()
    a.ntensors, a.nblocks = nt, len(c.bt)
    if not only_g:
        a.lr, a.beta1, a.beta2, a.eps, a.weight_decay, a.ema_decay = hp.lr, hp.b1, hp.b2, hp.eps, hp.wd, hp.decay
        a.ema_on_skip = hp.ema_on_skip
        if hp.found is not None:
            m.found = torch.full((), hp.found, dtype=F32, device=gpu)
            a.found_inf = m.found.data_ptr()
    m.a = a
    return m


def _aw_read(m):
    torch.cuda.synchronize()
    _intact(m.steps, "adamw step counters")
    outs = []
    for i, (T, fr) in enumerate(zip(m.c.ts, m.fr)):
        for k, f in fr.items():
            if f is not None:
                _intact(f, f"adamw tensor {i} {k}")
        step = m.steps.view[i].cpu()
        if T.step is None:
            assert bool(step.isnan()), "a counter behind a NULL step pointer was written"
        outs.append(NS(p=fr["p"].view.cpu(), m=fr["m"].view.cpu(), v=fr["v"].view.cpu(), ema=None if fr["ema"] is None else fr["ema"].view.cpu(),
                       step=None if T.step is None else step))
    return outs


def _aw_run(gpu, c, hp, **kw):
    m = _aw_build(gpu, c, hp, **kw)
    _ok("dm_adamw_ema_step", m.a)
    outs = _aw_read(m)
    aw_eval(c, hp, outs)
    return outs


def _aw_case():
    return aw_case(seed=5, chunk=_chunk())


def test_adamw_hyperparameters_null_rows_and_shuffled_blocks(gpu):
    """Tensor sizes 1, 3, 4, 5, 1023, chunk, chunk + 1, 2 chunk + 3 with the blocks listed in a shuffled order; one row with
    ema == NULL and one with step == NULL among full rows; counters 0, 9, 999, 99 999 (checked after the call); lr 1e-4 and 1e-2,
    weight decay 0 and 0.01, ema_decay 0, 0.25, 0.5, 0.9, 0.999, 0.9999, 1 (0: ema == p, 1: ema unchanged, bit for bit); gradients
    from 1e-20 to 1e4 over carried-over moments, g = m = v = 0 leaves the weight exactly; found_inf NULL and 0."""
    c = _aw_case()
    assert sorted(set(float(T.step) for T in c.ts if T.step is not None)) == [0.0, 9.0, 999.0, 99999.0]
    assert any(T.ema is None for T in c.ts) and any(T.step is None for T in c.ts)
    for hp in aw_hps():
        if hp.found != 1.0:
            _aw_run(gpu, c, hp)


def test_adamw_single_pointer_misalignment(gpu, capsys):
    """Each of p, m, v, g, ema one element off a 16-byte boundary on its own (the vector arm is chosen from p | m | v | g | ema): the
    element-wise arm within bound like the all-aligned run; whether the two agree bit for bit is reported, not demanded."""
    c = _aw_case()
    hp = aw_hp(lr=1e-2, wd=0.01, decay=0.9)
    base = _aw_run(gpu, c, hp)
    for k in AW_NAMES:
        outs = _aw_run(gpu, c, hp, mis=k)
        same = all(bits_equal(getattr(o, f), getattr(b, f)) for o, b in zip(outs, base) for f in ("p", "m", "v", "ema") if getattr(o, f) is not None)
        with capsys.disabled():
            print(f"adamw: {k} misaligned: bit-identical to the aligned run: {same}")


def test_adamw_skipped_step(gpu):
    """found_inf = 1 with g full of NaN: p, m, v and the counters bit-unchanged; ema moves towards the unchanged weights with
    ema_on_skip and is bit-unchanged without."""
    c = _aw_case()
    for on in (0, 1):
        for dec in (0.9, 0.9999, 0.25):
            outs = _aw_run(gpu, c, aw_hp(decay=dec, found=1.0, ema_on_skip=on), g_nan=True)
            moved = any(not bits_equal(o.ema, T.ema) for o, T in zip(outs, c.ts) if T.ema is not None)
            assert moved == bool(on)


def test_adamw_status_codes_write_nothing(gpu):
    from diffma_amd import _lib

    c = _aw_case()
    for kw in (dict(tensors=0), dict(block_tensor=0), dict(block_chunk=0), dict(ntensors=0), dict(nblocks=0), dict(beta1=1.0),
               dict(beta2=-0.1), dict(eps=-1.0), dict(ema_decay=1.5)):
        m = _aw_build(gpu, c, aw_hp())
        before = [(f.buf.clone()) for fr in m.fr for f in fr.values() if f is not None] + [m.steps.buf.clone()]
        for k, v in kw.items():
            setattr(m.a, k, v)
        assert _raw("dm_adamw_ema_step", m.a) == DM_ERR_ARG, kw
        torch.cuda.synchronize()
        after = [f.buf for fr in m.fr for f in fr.values() if f is not None] + [m.steps.buf]
        assert all(bits_equal(x, y) for x, y in zip(before, after)), kw
    assert int(_lib.load().dm_adamw_ema_step(None, None)) == DM_ERR_ARG
    assert int(_lib.load().dm_grads_nonfinite(None, None)) == DM_ERR_ARG


def test_fused_adamw_ema_wrapper_skips_a_parameter_without_gradient(gpu):
    """optim.FusedAdamWEMA with a parameter whose .grad is None between two that have one: the EMA rows pair with the right
    parameters (within bound of fp64), and the idle parameter, its EMA and its counter stay untouched."""
    from diffma_amd import optim

    g = torch.Generator().manual_seed(11)
    sizes = [37, 5, 4099]
    p0 = [torch.randn(n, generator=g) for n in sizes]
    e0 = [p + 0.5 * torch.randn(n, generator=g) for p, n in zip(p0, sizes)]
    gr = [torch.randn(n, generator=g) for n in sizes]
    ps = [torch.nn.Parameter(p.clone().to(gpu)) for p in p0]
    es = [e.clone().to(gpu) for e in e0]
    opt = torch.optim.AdamW(ps, lr=1e-2, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)
    fused = optim.FusedAdamWEMA(opt, ps, es, ema_decay=0.9)
    ps[0].grad, ps[2].grad = gr[0].to(gpu), gr[2].to(gpu)
    fused.step()
    torch.cuda.synchronize()
    z = lambda n: torch.zeros(n)
    c = NS(ts=[NS(n=sizes[i], p=p0[i], m=z(sizes[i]), v=z(sizes[i]), g=gr[i], ema=e0[i], step=torch.tensor(0.0)) for i in (0, 2)])
    outs = [NS(p=ps[i].detach().cpu(), m=opt.state[ps[i]]["exp_avg"].cpu(), v=opt.state[ps[i]]["exp_avg_sq"].cpu(), ema=es[i].cpu(),
               step=opt.state[ps[i]]["step"].cpu()) for i in (0, 2)]
    aw_eval(c, aw_hp(lr=1e-2, wd=0.01, decay=0.9), outs)
    assert bits_equal(ps[1].detach().cpu(), p0[1]) and bits_equal(es[1].cpu(), e0[1]) and float(opt.state[ps[1]]["step"]) == 0.0
    assert not bool(opt.state[ps[1]]["exp_avg"].any())


# =====================================================================================================================================
# dm_grads_nonfinite
# =====================================================================================================================================
def _nf_table(gpu, gs, aligned):
    c = aw_case(seed=5, chunk=_chunk())
    for T, x in zip(c.ts, gs):
        T.g = x
    m = _aw_build(gpu, c, None, mis=None if aligned else "g", only_g=True)
    m.flag = _frame(gpu, F32, 1, fill=torch.zeros(1))
    m.a.nonfinite_out = m.flag.view.data_ptr()
    return m


def _nf_call(m):
    m.flag.view.zero_()
    _ok("dm_grads_nonfinite", m.a)
    torch.cuda.synchronize()
    _intact(m.flag, "grads_nonfinite flag")
    return float(m.flag.view[0])


@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "misaligned"])
def test_grads_nonfinite_every_position(gpu, aligned):
    """Only g, the table and the block arrays set.  All-finite gradients (+-3.4e38, denormals, -0.0 among them) leave 0; one +Inf, -Inf
    or NaN at the first element, each lane of a vector, the last element of a chunk, the first of the next, each element of an n % 4
    tail, the last tensor of the table -- each sets 1; a non-finite value in the frame just past n leaves 0."""
    gs = nf_case()
    m = _nf_table(gpu, gs, aligned)
    nf_eval(gs, _nf_call(m))
    assert _nf_call(m) == 0.0
    for ti, i in nf_positions(_chunk()):
        view = m.fr[ti]["g"].view
        old = float(view[i])
        for val in (INF, -INF, NAN):
            view[i] = val
            planted = [x.clone() for x in gs]
            planted[ti][i] = val
            got = _nf_call(m)
            nf_eval(planted, got)
            assert got == 1.0, (ti, i, val)
        view[i] = old
    assert _nf_call(m) == 0.0
    for fr in m.fr:                                              # the element just past n belongs to the frame
        f = fr["g"]
        for val in (INF, NAN):
            f.buf[f.off + f.n] = val
            assert _nf_call(m) == 0.0
            f.buf[f.off + f.n] = SENT


def test_grads_nonfinite_null_output(gpu):
    m = _nf_table(gpu, nf_case(), True)
    m.a.nonfinite_out = 0
    assert _raw("dm_grads_nonfinite", m.a) == DM_ERR_ARG
    torch.cuda.synchronize()
    assert float(m.flag.view[0]) == 0.0


def test_zz_error_to_bound_ratios(gpu):
    """Prints the largest error-to-bound ratio per operator and dtype that the tests of this file have seen so far (run it with -s)."""
    for k in sorted(RATIOS):
        print(f"gpu ratio {k[0]:18s} {k[1]}: {RATIOS[k]:.3f}")
    assert all(v <= 1.0 for v in RATIOS.values())
