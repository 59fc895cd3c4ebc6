"""Do two builds of the kernels compute the same bits in the Mamba-2 SSD forward?  Run on the GPU box.
    tools/ssd_fwd_same_bits.py LIB_A LIB_B [--out result.json]
For each libdiffma_hip.so one fresh child process (DIFFMA_HIP_LIB names the library it loads) runs the case list below through
hip_ops.ssd_fwd / hip_ops.ssd_fwd_chunked and saves every framed output buffer as int16; this process compares the two files case by
case (numpy.array_equal) and prints the count of differing cases.  Inputs: the builders of tests/test_ssd_gpu.py (d_state 16),
tests/test_ssd_wide_cpu.py and tests/test_ssd_chunked_cpu.py (three directions where the length has them, row-index tables, the randn
family), views as in tests/test_ssd_chunked_gpu._launch.

Cases (Q = dm_ssd_fwd_chunk_len(d_state)):
    dm_ssd_fwd          d_state 16             L 1, 33, 196, 224 x bf16, f16, 4 heads; L 33 without a gate
    dm_ssd_fwd          d_state 32 / 64 / 128  L 33, 196, 224 x bf16, f16 x 4 and 3 heads; bf16 L 33: gate rows on 4-byte boundaries (2 heads), no gate
    dm_ssd_fwd_chunked  all four widths        L 1, Q, Q + 1, 2 Q + 33 x bf16, f16 x 4 and 3 heads; bf16 2 Q + 33: the 4-byte gate (2 heads), no gate;
                                               L 1024 at d_state 16 and 128
"""
import argparse, json, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def cases(chunk_len):
    """(entry, N, L, dtype name, heads, gate: 'z' | 'z4' (rows on 4-byte boundaries) | 'none')"""
    out = []
    for dt in ("bf16", "f16"):
        out += [("ssd_fwd", 16, L, dt, 4, "z") for L in (1, 33, 196, 224)] + [("ssd_fwd", 16, 33, dt, 4, "none")]
    for N in (32, 64, 128):
        out += [("ssd_fwd", N, L, dt, nh, "z") for L in (33, 196, 224) for dt in ("bf16", "f16") for nh in (4, 3)]
        out += [("ssd_fwd", N, 33, "bf16", 2, "z4"), ("ssd_fwd", N, 33, "bf16", 4, "none")]
    for N in (16, 32, 64, 128):
        Q = chunk_len(N)
        out += [("ssd_fwd_chunked", N, L, dt, nh, "z") for L in (1, Q, Q + 1, 2 * Q + 33) for dt in ("bf16", "f16") for nh in (4, 3)]
        out += [("ssd_fwd_chunked", N, 2 * Q + 33, "bf16", 2, "z4"), ("ssd_fwd_chunked", N, 2 * Q + 33, "bf16", 4, "none")]
    out += [("ssd_fwd_chunked", N, 1024, dt, 4, "z") for N in (16, 128) for dt in ("bf16", "f16")]
    return out


def child(path):
    import numpy as np
    import torch

    from diffma_amd import _lib, hip_ops
    from tests import test_ssd_chunked_cpu as chunked_cpu
    from tests import test_ssd_gpu as d16
    from tests import test_ssd_wide_cpu as wide_cpu

    gpu = torch.device("cuda", 0)
    NAN, SENT, P = d16.NAN, d16.SENT, d16.P
    saved = {}
    for entry, N, L, dt, nh, gate in cases(chunked_cpu.chunk_len):
        dtype = torch.bfloat16 if dt == "bf16" else torch.float16
        if entry == "ssd_fwd_chunked":
            c = chunked_cpu.inputs(L, dtype, N, nh)
        elif N == 16:
            c = d16._inputs(L, dtype)
        else:
            c = wide_cpu.inputs(L, dtype, N, nh)
        S, din = c["S"], nh * P
        xb = torch.full((S, L + 4, din + 2 * N + 8), NAN, dtype=dtype, device=gpu)
        xb[:, 2:2 + L, :din + 2 * N] = c["xBC"].to(gpu)
        v = xb[:, 2:2 + L]
        x, Bm, Cm = v[..., :din], v[..., din:din + N], v[..., din + N:din + 2 * N]
        z = None
        if gate != "none":
            zb = torch.full((c["bpd"], L, din + (2 if gate == "z4" else 0)), NAN, dtype=dtype, device=gpu)
            zb[..., :din] = c["z"].to(gpu)
            z = zb[..., :din]
        buf = torch.full((S, L + 4, din + 8), SENT, dtype=dtype, device=gpu)
        view = buf[:, 2:2 + L, :din]
        view.fill_(NAN)
        A, D, bias = (t.float().to(gpu) for t in wide_cpu.head_params(nh))
        getattr(hip_ops, entry)(x, Bm, Cm, c["dt_tok"].to(gpu), z, A, D, bias, out=view, z_row_index=c["zperm"].int().to(gpu),
                                out_row_index=c["operm"].int().to(gpu), batch_per_dir=c["bpd"])
        torch.cuda.synchronize()
        assert not bool(torch.isnan(view.float()).any()), (entry, N, L, dt, nh, gate)
        saved[f"{entry} N{N} L{L} {dt} H{nh} {gate}"] = buf.view(torch.int16).cpu().numpy()
    np.savez(path, **saved)
    print(f"CHILD {len(saved)} cases, library {_lib.LIB_PATH}", flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("libs", nargs="*", help="two libdiffma_hip.so")
    ap.add_argument("--child", default="", help="(internal) run the cases with the library of DIFFMA_HIP_LIB and save them here")
    ap.add_argument("--out", default="", help="write the result as JSON")
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    assert len(a.libs) == 2, "two libraries"
    import tempfile

    import numpy as np

    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for k, lib in enumerate(a.libs):
            files.append(os.path.join(tmp, f"lib{k}.npz"))
            env = dict(os.environ, DIFFMA_HIP_LIB=os.path.abspath(lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", files[-1]], env=env, capture_output=True, text=True, timeout=a.timeout)
            if p.returncode != 0 or not os.path.exists(files[-1]):   # stop: nothing more is started on a device that has just failed a run
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                raise SystemExit(f"{lib}: child failed with exit status {p.returncode}")
            print(p.stdout.strip().splitlines()[-1], flush=True)
        fa, fb = (np.load(f) for f in files)
        assert sorted(fa.files) == sorted(fb.files)
        differing = [k for k in fa.files if not np.array_equal(fa[k], fb[k])]
    res = dict(libraries=a.libs, cases=len(fa.files), differing_cases=len(differing), differing=differing)
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
