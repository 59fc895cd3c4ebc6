"""Forced-variant A/B of the scan kernels: the sequential-in-lane kernels (K1 / K2) against the time-parallel
two-pass kernels (K1c / K2c, the north star's "wave-parallel" form) in the mixer's call pattern -- bf16 I/O, three directions
through row-index tables, no z, delta already activated, checkpoints for the backward.  Kernel-only times (events around the C-ABI
launch): the two variants alternate launch by launch in one process, and every figure is the median over --iters timed launches
after --warmup untimed ones, with the spread (min, 10th and 90th percentile, max) beside it.

Both scans are chunk-parallel up to 1024 tokens: one segment up to 196, segments of dm_scan_fwd_launch_segment /
dm_scan_bwd_launch_segment tokens past that.  A "chunked" arm is timed wherever the forced query answers for it; the backward reads
the checkpoints of the sequential forward in both arms (either forward writes the same slots).

--sample-step SIZE times the graphed and the eager batch-1 denoiser call of DiffMa-L/2 at input_size SIZE with the forward's switch
(DIFFMA_SCAN_CHUNKED_LONG) on and off, --train-step SIZE the graphed one-sample training step with the backward's switch
(DIFFMA_SCAN_BWD_CHUNKED_LONG) on and off; the two arms alternate call by call in one process and are compared with each other.

  python tools/scan_variants.py [--nseq 1536 768 96 24] [--iters 10]  > profiles/r04_scan_variants.txt
  python tools/scan_variants.py --forward-only --seqlen 256 1024 --dim 1024 2048 --nseq 3 24 96 192 --iters 50 \
         --sample-step 32 64 --json profiles/scan_fwd_chunked_long.json
  python tools/scan_variants.py --seqlen 256 1024 --dim 1024 2048 --nseq 3 6 15 24 48 96 --iters 50 \
         --train-step 32 64 --json profiles/scan_bwd_chunked_long.json
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffma_amd import _lib, hip_ops  # noqa: E402


def spread(us):
    us = sorted(us)
    q = lambda f: us[min(len(us) - 1, int(f * len(us)))]
    return dict(median=round(q(0.5), 1), min=round(us[0], 1), p10=round(q(0.1), 1), p90=round(q(0.9), 1), max=round(us[-1], 1), n=len(us))


def kernel_us(fns, name, iters, warmup):
    """fns: {label: launch}.  The launches alternate (a, b, a, b, ...); returns {label: spread of the per-launch kernel times}."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    tms = {k: hip_ops.KernelTimer() for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            prev = hip_ops.set_timer(tms[k])
            fn()
            hip_ops.set_timer(prev)
    torch.cuda.synchronize()
    return {k: spread([1e3 * r[0].elapsed_time(r[1]) for r in tm.records[name]]) for k, tm in tms.items()}


def scan_rows(a, dev):
    N, dt = 16, torch.bfloat16
    rows = []
    for L in a.seqlen:
        for Dm in a.dim:
            for S in a.nseq:
                Bd = S // 3
                g = torch.Generator(device=dev).manual_seed(S)
                mk = lambda *s: torch.randn(*s, device=dev, generator=g)
                u, Bm, Cm = mk(S, L, Dm).to(dt), mk(S, L, N).to(dt), mk(S, L, N).to(dt)
                bias = mk(Dm) * 0.5
                act = torch.nn.functional.softplus(mk(S, L, Dm) * 0.5 + bias).to(dt)
                A, Dp = -(torch.rand(Dm, N, device=dev, generator=g) * 4 + 0.2), mk(Dm)
                idx = torch.stack([torch.arange(L), torch.randperm(L), torch.randperm(L)]).to(torch.int32).to(dev)
                out = torch.empty_like(u)
                kw = dict(z_row_index=idx, out_row_index=idx, batch_per_dir=Bd, delta_activated=True)
                seg = hip_ops.scan_fwd_segment(S, Dm, L, N, _lib.DM_FLAG_SCAN_CHUNKED)
                row = dict(nseq=S, L=L, D=Dm, N=N, dtype="bf16", fwd_segment=seg, fwd_routed_chunked=hip_ops.scan_fwd_segment(S, Dm, L, N, 0) > 0)
                fwd_variants = ("sequential", "chunked") if seg > 0 else ("sequential",)
                ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Dm, dt, dev)
                fwd = lambda v, ck: (lambda: hip_ops.scan_fwd(u, act, A, Bm, Cm, Dp, None, bias, True, out=out, ckpt=ck, variant=v, **kw))
                for label, ck in (("fwd_ckpt", ckpt), ("fwd_nockpt", None)):
                    t = kernel_us({v: fwd(v, ck) for v in fwd_variants}, "dm_selective_scan_fwd", a.iters, a.warmup)
                    for v in fwd_variants:
                        row[f"{label}_{v}_us"] = t[v]["median"]
                        row[f"{label}_{v}_spread"] = t[v]
                    if "chunked" in t:
                        row[f"{label}_speedup"] = round(t["sequential"]["median"] / t["chunked"]["median"], 3)
                if not a.forward_only:
                    dout = mk(Bd, L, Dm).to(dt)
                    # the chunk-parallel backward writes one dB/dC partial row per 64 channels: that is how the library tells
                    bwd_variants = ("sequential", "chunked") if _lib.load().dm_scan_bwd_launch_group_channels(S, Dm, L, N, _lib.DM_FLAG_SCAN_CHUNKED) == 64 else ("sequential",)
                    fwd("sequential", ckpt)()
                    bwd = lambda v: (lambda: hip_ops.scan_bwd(u, act, A, Bm, Cm, Dp, None, bias, dout, ckpt, True, variant=v, **kw))
                    t = kernel_us({v: bwd(v) for v in bwd_variants}, "dm_selective_scan_bwd", a.iters, a.warmup)
                    for v in bwd_variants:
                        row[f"bwd_{v}_us"] = t[v]["median"]
                        row[f"bwd_{v}_spread"] = t[v]
                    row["bwd_segment"] = hip_ops.scan_bwd_segment(S, Dm, L, N, _lib.DM_FLAG_SCAN_CHUNKED)
                    row["bwd_routed_chunked"] = hip_ops.scan_bwd_segment(S, Dm, L, N, 0) > 0
                    if "chunked" in t:
                        row["bwd_speedup"] = round(t["sequential"]["median"] / t["chunked"]["median"], 3)
                del ckpt
                print(json.dumps(row), flush=True)
                rows.append(row)
    return rows


def sample_step_rows(a, dev):
    """One batch-1 denoiser call of DiffMa-L/2 under bf16 autocast (what a p_sample step runs), eager and as a hipGraph replay, with
    the chunk-parallel forward past 196 tokens on and off (hip_ops.SCAN_CHUNKED_LONG = DIFFMA_SCAN_CHUNKED_LONG), alternating."""
    from diffma_amd.graphed import GraphedDenoiser
    from diffma_amd.model import DiffMa_models

    rows = []
    for size in a.sample_step:
        torch.manual_seed(size)
        net = DiffMa_models["DiffMa-L/2"](input_size=size).to(dev).eval()
        L = (size // 2) ** 2
        x, t = torch.randn(1, 4, size, size, device=dev), torch.tensor([500], device=dev)
        y, y2, w = torch.randn(1, 512, device=dev), torch.randn(1, L, 512, device=dev), torch.rand(1, L, 1, device=dev)
        graphs = {}
        for on in (True, False):
            hip_ops.SCAN_CHUNKED_LONG = on
            graphs[on] = GraphedDenoiser(net, x, t, y, y2, w, autocast_dtype=torch.bfloat16)

        def eager(on):
            hip_ops.SCAN_CHUNKED_LONG = on
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                net(x, t, y=y, y2=y2, w=w)

        row = dict(model="DiffMa-L/2", input_size=size, L=L, batch=1, dtype="bf16 autocast")
        for mode, call in (("eager", eager), ("graph", lambda on: graphs[on](x, t, y=y, y2=y2, w=w))):
            times = {True: [], False: []}
            for i in range(a.warmup + a.iters):
                for on in (True, False):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    call(on)
                    e1.record()
                    torch.cuda.synchronize()
                    if i >= a.warmup:
                        times[on].append(1e3 * e0.elapsed_time(e1))
            row[f"{mode}_chunked_long_us"], row[f"{mode}_sequential_us"] = spread(times[True]), spread(times[False])
            row[f"{mode}_speedup"] = round(row[f"{mode}_sequential_us"]["median"] / row[f"{mode}_chunked_long_us"]["median"], 3)
        hip_ops.SCAN_CHUNKED_LONG = True
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def train_step_rows(a, dev):
    """The graphed one-sample training step of DiffMa-L/2 under bf16 autocast (graphed.GraphedTrainStep: noise, forward, loss, backward,
    fused AdamW, EMA in one hipGraph), captured once with the chunk-parallel backward past 196 tokens on and once with it off
    (hip_ops.SCAN_BWD_CHUNKED_LONG = DIFFMA_SCAN_BWD_CHUNKED_LONG; the flag word is fixed at capture).  Each arm steps its own copy
    of the model; the replays alternate."""
    import copy

    from diffma_amd.diffusion import create_diffusion
    from diffma_amd.graphed import GraphedTrainStep
    from diffma_amd.model import DiffMa_models

    rows = []
    diffusion = create_diffusion("")
    for size in a.train_step:
        L = (size // 2) ** 2
        g = torch.Generator(device=dev).manual_seed(size)
        mk = lambda *s: torch.randn(*s, device=dev, generator=g)
        z, y, y2, w = mk(1, 4, size, size), mk(1, 512), mk(1, L, 512), torch.sigmoid(mk(1, L, 1))
        t = torch.tensor([500], device=dev)
        steps = {}
        for on in (True, False):
            hip_ops.SCAN_BWD_CHUNKED_LONG = on
            torch.manual_seed(size)
            model = DiffMa_models["DiffMa-L/2"](input_size=size).to(dev).train()
            ema = copy.deepcopy(model).requires_grad_(False)
            opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0, fused=True, capturable=True)
            steps[on] = GraphedTrainStep(model, ema, opt, diffusion, z, t, y, y2, w, autocast_dtype=torch.bfloat16, ema_decay=0.999)
        hip_ops.SCAN_BWD_CHUNKED_LONG = True
        times = {True: [], False: []}
        for i in range(a.warmup + a.iters):
            for on in (True, False):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                steps[on].step(z, t, y, y2, w)
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    times[on].append(1e3 * e0.elapsed_time(e1))
        d_inner = 2 * 1024
        row = dict(model="DiffMa-L/2", input_size=size, L=L, batch=1, dtype="bf16 autocast", mode="graphed training step",
                   bwd_segment=hip_ops.scan_bwd_segment(3, d_inner, L, 16, 0),
                   graph_bwd_chunked_long_us=spread(times[True]), graph_bwd_sequential_us=spread(times[False]))
        row["graph_speedup"] = round(row["graph_bwd_sequential_us"]["median"] / row["graph_bwd_chunked_long_us"]["median"], 3)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del steps
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nseq", type=int, nargs="+", default=[1536, 768, 96, 24])
    ap.add_argument("--seqlen", type=int, nargs="+", default=[196])
    ap.add_argument("--dim", type=int, nargs="+", default=[1024])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forward-only", action="store_true", help="time the forward alone")
    ap.add_argument("--sample-step", type=int, nargs="*", default=[], metavar="INPUT_SIZE",
                    help="also time one batch-1 DiffMa-L/2 denoiser call at these input sizes, DIFFMA_SCAN_CHUNKED_LONG on against off")
    ap.add_argument("--train-step", type=int, nargs="*", default=[], metavar="INPUT_SIZE",
                    help="also time the graphed one-sample DiffMa-L/2 training step at these input sizes, DIFFMA_SCAN_BWD_CHUNKED_LONG on against off")
    ap.add_argument("--json", default=None, help="write everything to this file as one JSON document")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    doc = dict(device=torch.cuda.get_device_name(0), iters=a.iters, warmup=a.warmup,
               note="kernel times in us from device events around the C-ABI launch, variants alternating in one process",
               scans=scan_rows(a, dev), sample_step=sample_step_rows(a, dev), train_step=train_step_rows(a, dev))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
