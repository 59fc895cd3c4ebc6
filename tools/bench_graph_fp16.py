#!/usr/bin/env python
"""Step time of the graphed training step in fp16 with the loss scale on the device, next to what it has to be compared with.

    python tools/bench_graph_fp16.py [--parent-lib PATH/libdiffma_hip.so] [--rounds 3] [--steps 50] [--out profiles/graph_fp16_step.json]

DiffMa-L/2, ONE sample, 196 tokens (the reference's config/brain.yaml per GPU).  Arms, each a fresh process so that a kernel library
can be swapped, run in alternation (arm 1, arm 2, ..., arm 1, arm 2, ...) `--rounds` times:
    bf16          graphed bf16 step, this build
    bf16_parent   graphed bf16 step, the library given with --parent-lib (the parent commit's build; skipped without it)      (a)
    fp16_plain    graphed fp16 step, loss_scale=None (trains unscaled: a timing baseline only)                                  (b)
    fp16_scaled   graphed fp16 step with optim.DeviceLossScale                                                                  (c)
    fp16_eager    the eager fp16 loop of train.py: DDP wrapper, GradScaler, per-step host read of the loss                      (d)
                  (a copy of the accepted-step arm of train.main's loop body, kept here by hand: compare it with train.py when
                  that loop changes)
A run is `--steps` steps between two device synchronisations after `--warmup` untimed ones; the figure of an arm is the median of
its runs, its spread their (max - min).  An older library knows neither dm_loss_scale_update nor ABI 37: the bf16_parent arm binds the
functions that library has and accepts its ABI number (the bf16 path passes no field the older struct lacks).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
ARMS = ("bf16", "bf16_parent", "fp16_plain", "fp16_scaled", "fp16_eager")


def child(arm, steps, warmup):
    import ctypes

    import torch

    from diffma_amd import _lib
    if arm == "bf16_parent":
        old = ctypes.CDLL(_lib.LIB_PATH)
        _lib.FUNCTIONS = [f for f in _lib.FUNCTIONS if hasattr(old, f[1])]
        _lib.EXPORTED_SYMBOLS = [name for _, name, _ in _lib.FUNCTIONS]
        _lib.ARGTYPES = {name: _lib.ARGTYPES[name] for name in _lib.EXPORTED_SYMBOLS}
        _lib.CONSTANTS["DM_ABI_VERSION"] = int(old.dm_abi_version())
    from diffma_amd import train as T
    from diffma_amd.diffusion import create_diffusion
    from diffma_amd.gemm_tuning import enable_tuned_gemms
    from diffma_amd.graphed import GraphedTrainStep
    from diffma_amd.model import DiffMa_models
    from diffma_amd.optim import DeviceLossScale

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    enable_tuned_gemms()
    model = DiffMa_models["DiffMa-L/2"](input_size=28, dt_rank=16, d_state=16).to(dev)
    with torch.no_grad():                                       # the zero-initialised tensors would leave most of the backward idle
        for p in model.parameters():
            if float(p.abs().max()) == 0.0:
                p.normal_(0, 0.02)
    from copy import deepcopy
    ema = deepcopy(model).requires_grad_(False)
    d = create_diffusion("")
    g = torch.Generator(device=dev).manual_seed(1)
    mk = lambda *s: torch.randn(*s, generator=g, device=dev)
    z, y, y2, w = mk(1, 4, 28, 28), mk(1, 512), mk(1, 196, 512), torch.sigmoid(mk(1, 196, 1))
    amp = torch.bfloat16 if arm.startswith("bf16") else torch.float16
    info = {}
    if arm == "fp16_eager":
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if "MASTER_PORT" not in os.environ:
            import socket
            with socket.socket() as sock:                       # a free port, as the tests pick one
                sock.bind(("127.0.0.1", 0))
                os.environ["MASTER_PORT"] = str(sock.getsockname()[1])
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
        ddp = T.wrap_ddp(model, dev)
        opt = torch.optim.AdamW(ddp.parameters(), lr=1e-4, weight_decay=0, fused=True)
        scaler = torch.amp.GradScaler("cuda")
        ddp.train()

        def step():                                             # the accepted-step arm of train.main's eager loop
            t = torch.randint(0, d.num_timesteps, (1,), device=dev)
            with torch.autocast("cuda", dtype=amp):
                loss = d.training_losses(ddp, z, t, dict(y=y, y2=y2, w=w))["loss"].mean()
            lv = loss.detach().float()
            flag = torch.stack([(~torch.isfinite(lv)).float(), torch.nan_to_num(lv, nan=0.0, posinf=0.0, neginf=0.0)])
            flag.tolist()
            scaler.scale(loss).backward()
            scaler.step(opt)
            scaler.update()
            T.update_ema(ema, model)
            opt.zero_grad(set_to_none=True)
    else:
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0, fused=True, capturable=True)
        model.train()
        ls = DeviceLossScale(dev) if arm == "fp16_scaled" else None
        kw = {} if ls is None else dict(loss_scale=ls)
        gs = GraphedTrainStep(model, ema, opt, d, z, torch.zeros(1, device=dev, dtype=torch.long), y, y2, w, autocast_dtype=amp, ema_decay=0.999, **kw)

        def step():
            gs.step(z, torch.randint(0, d.num_timesteps, (1,), device=dev), y, y2, w)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    if arm == "fp16_eager":
        info["scale"] = scaler.get_scale()
        torch.distributed.destroy_process_group()
    elif arm != "bf16_parent":
        info["skipped"] = float(gs.skipped)
        if ls is not None:
            info["scale"] = float(ls.scale)
    print("RESULT " + json.dumps(dict(arm=arm, ms_per_step=ms, steps=steps, abi=int(_lib.load().dm_abi_version()), **info)), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--arm", choices=ARMS, help="(internal) measure one arm in this process")
    ap.add_argument("--parent-lib", default="", help="libdiffma_hip.so of the parent commit, for arm (a)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per arm process")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "graph_fp16_step.json"))
    a = ap.parse_args()
    if a.arm:
        return child(a.arm, a.steps, a.warmup)
    arms = [x for x in ARMS if x != "bf16_parent" or a.parent_lib]
    runs = {x: [] for x in arms}
    notes = {}
    for r in range(a.rounds):
        for arm in arms:
            env = dict(os.environ)
            env.pop("DIFFMA_HIP_LIB", None)
            if arm == "bf16_parent":
                env["DIFFMA_HIP_LIB"] = os.path.abspath(a.parent_lib)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--arm", arm, "--steps", str(a.steps), "--warmup", str(a.warmup)],
                               env=env, capture_output=True, text=True, timeout=a.timeout)
            line = next((l for l in p.stdout.splitlines() if l.startswith("RESULT ")), None)
            if p.returncode != 0 or line is None:                # stop: nothing more is started on a device that has just failed a run
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"arm {arm} failed with exit status {p.returncode}")
            rec = json.loads(line[7:])
            runs[arm].append(rec["ms_per_step"])
            notes[arm] = {k: v for k, v in rec.items() if k not in ("arm", "ms_per_step")}
            print(f"round {r} {arm:12s} {rec['ms_per_step']:8.3f} ms/step  {notes[arm]}", flush=True)
    out = dict(workload="DiffMa-L/2, 1 sample, 196 tokens, one MI355X; ms per training step; fp16_eager is a hand copy of the "
                        "accepted-step arm of train.main's eager loop, not that loop itself", rounds=a.rounds, steps=a.steps, warmup=a.warmup,
               arms={x: dict(median_ms=statistics.median(v), spread_ms=max(v) - min(v), runs_ms=v, **notes[x]) for x, v in runs.items()})
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
