"""Mamba-2 SSD forward on the matrix pipe (K6) against the A-shared scan at the DiffMa-XL/2 --use-mamba2 shape -- run on the GPU box.
    tools/bench_ssd.py [--d-state N] [--seqlen L] [batch ...]      N in 16 (default) / 32 / 64 / 128, L = 196 (default) .. 1024
Both pairs are timed at every width: dm_ssd_fwd against the A-shared scan forward, and the matrix-pipe backward (dm_ssd_bwd at 16,
dm_ssd_bwd_wide at 32 / 64 / 128, called through hip_ops.ssd_bwd whatever the routing switches say) against the A-shared scan
backward.  The backward pair alternates three windows of at least 0.1 s each and reports the medians and the spread.
Past L = 224 (--seqlen 256, --seqlen 1024: the 256- and 512-pixel image sizes) the forward pair is dm_ssd_fwd_chunked against the A-shared
scan forward, timed the same way (alternating windows, medians, spread); there is no matrix-pipe backward at those lengths."""
import argparse, os, sys, json
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from diffma_amd import hip_ops  # noqa: E402

dev = torch.device("cuda", 0)
ap = argparse.ArgumentParser()
ap.add_argument("--d-state", type=int, default=16)
ap.add_argument("--seqlen", type=int, default=196)
ap.add_argument("batches", nargs="*", type=int, default=[8, 64, 256])
args = ap.parse_args()
L, H, P, N = args.seqlen, 16, 64, args.d_state
CHUNKED = L > 224
Din = H * P
dt_ = torch.bfloat16


def timeit(fn, iters=int(os.environ.get("SSD_ITERS", "30"))):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


for B in args.batches:
    S = 3 * B
    xBC = torch.randn(S, L, Din + 2 * N, device=dev).to(dt_)
    dt_tok = (torch.randn(B, L, H, device=dev) * 0.7 - 1.0).to(dt_)
    z = torch.randn(B, L, Din, device=dev).to(dt_)
    A_h = -(torch.rand(H, device=dev) * 6 + 0.3)
    D_h, b_h = torch.randn(H, device=dev), torch.randn(H, device=dev) * 0.5
    idx = torch.stack([torch.arange(L), torch.randperm(L), torch.randperm(L)]).int().to(dev)
    x, Bm, Cm = xBC[..., :Din], xBC[..., Din:Din + N], xBC[..., Din + N:]
    out = torch.empty(S, L, Din, device=dev, dtype=dt_)

    def mfma():
        return (hip_ops.ssd_fwd_chunked if CHUNKED else hip_ops.ssd_fwd)(x, Bm, Cm, dt_tok, z, A_h, D_h, b_h, z_row_index=idx, out_row_index=idx, batch_per_dir=B, out=out)

    A = A_h.repeat_interleave(P)[:, None].expand(Din, N).contiguous()
    Dp, bp = D_h.repeat_interleave(P), b_h.repeat_interleave(P)
    idx64 = idx.long()

    def scan():
        dtg = torch.stack([dt_tok[:, idx64[k]] for k in range(3)]).reshape(S, L, H, 1).expand(S, L, H, P).reshape(S, L, Din)
        return hip_ops.scan_fwd(x, dtg, A, Bm, Cm, Dp, z, bp, True, z_row_index=idx, out_row_index=idx, batch_per_dir=B, a_shared=True, out=out)

    def bench_bwd():
        # ---- backward: K6b against the A-shared scan backward (which also needs the forward's checkpoints and the expanded delta) ----
        dout = torch.randn(S, L, Din, device=dev).to(dt_)
        dxBC = torch.empty_like(xBC)

        def mfma_bwd():
            return hip_ops.ssd_bwd(x, Bm, Cm, dt_tok, z, dout, A_h, D_h, b_h, z_row_index=idx, out_row_index=idx, batch_per_dir=B, dx_out=dxBC[..., :Din])

        dtg = torch.stack([dt_tok[:, idx64[k]] for k in range(3)]).reshape(S, L, H, 1).expand(S, L, H, P).reshape(S, L, Din)
        ckpt = hip_ops.alloc_scan_ckpt(S, L, N, Din, dt_, dev)
        hip_ops.scan_fwd(x, dtg, A, Bm, Cm, Dp, z, bp, True, z_row_index=idx, out_row_index=idx, batch_per_dir=B, a_shared=True, out=out, ckpt=ckpt)

        def scan_bwd():
            return hip_ops.scan_bwd(x, dtg, A, Bm, Cm, Dp, z, bp, dout, ckpt, True, z_row_index=idx, out_row_index=idx, batch_per_dir=B, dout_per_seq=True,
                                    du_out=dxBC[..., :Din], a_shared=True, dbc_out=dxBC[..., Din:])

        mfma_bwd()
        scan_bwd()
        iters = lambda fn: max(10, int(1e5 / timeit(fn, 5)))                   # a window of 0.1 s or more
        n_m, n_s = iters(mfma_bwd), iters(scan_bwd)
        t_mb, t_sb = [], []
        for _ in range(3):                                                     # alternate the two: other work shares the host
            t_mb.append(timeit(mfma_bwd, n_m))
            t_sb.append(timeit(scan_bwd, n_s))
        med = lambda v: sorted(v)[1]
        spread = lambda v: round((max(v) - min(v)) / med(v), 3)
        HG = 1 if N == 16 else hip_ops._lib.CONSTANTS["DM_SSD_BWD_WIDE_HEADS"]
        GC = 256 if N == 16 else 4096 // N                                     # channels per scan-backward launch group (README "Shapes")
        return dict(ssd_bwd_mfma_us=round(med(t_mb), 1), a_shared_scan_bwd_us=round(med(t_sb), 1), scan_bwd_over_mfma_bwd=round(med(t_sb) / med(t_mb), 2),
                    spread_mfma=spread(t_mb), spread_scan=spread(t_sb), mfma_dbc_workspace_bytes=-(-H // HG) * S * L * 8 * N,
                    scan_dbc_workspace_bytes=-(-Din // GC) * S * L * 8 * N)

    a = mfma().float().clone()
    b = scan().float()
    nb = 3 * S * L * Din * 2
    if CHUNKED:
        iters = lambda fn: max(10, int(1e5 / timeit(fn, 5)))                   # a window of 0.1 s or more
        n_m, n_s = iters(mfma), iters(scan)
        t_mf, t_sf = [], []
        for _ in range(3):                                                     # alternate the two: other work shares the host
            t_mf.append(timeit(mfma, n_m))
            t_sf.append(timeit(scan, n_s))
        med = lambda v: sorted(v)[1]
        t_m, t_s = med(t_mf), med(t_sf)
        print(json.dumps(dict(d_state=N, seqlen=L, batch=B, nseq=S, ssd_chunked_us=round(t_m, 1), a_shared_scan_us=round(t_s, 1), scan_over_chunked=round(t_s / t_m, 2),
                              spread_chunked=round((max(t_mf) - min(t_mf)) / t_m, 3), spread_scan=round((max(t_sf) - min(t_sf)) / t_s, 3),
                              chunk_len=hip_ops._lib.load().dm_ssd_fwd_chunk_len(N), chunked_GBps=round(nb / t_m / 1e3, 1),
                              max_abs_diff=float((a - b).abs().max()), scale=float(b.abs().max()))), flush=True)
        continue
    t_m, t_s = timeit(mfma), timeit(scan)
    res = dict(d_state=N, batch=B, nseq=S, ssd_mfma_us=round(t_m, 1), a_shared_scan_us=round(t_s, 1), scan_over_mfma=round(t_s / t_m, 2),
               mfma_GBps=round(nb / t_m / 1e3, 1), max_abs_diff=float((a - b).abs().max()), scale=float(b.abs().max()))
    res.update(bench_bwd())
    print(json.dumps(res), flush=True)
