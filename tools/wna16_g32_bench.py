"""Prompt-sized group-size-32 W4A16 GEMM (csrc/wna16_gemm_large_g32.hip, ops.wna16_gemm_large_g32) against what
ops.gptq_gemm(bit=4, use_exllama=True) runs for the same call without it (APHRO_WNA16_NO_LARGE=1): 64-row passes of the
decode kernel below GPTQ_DEQUANT_MIN_M rows, gptq_dequant + torch.matmul from there.  Both arms gather a[:, perm] (act-order).
Shapes: the four Llama-3-8B projections and the row-parallel projections of a 70B at TP 8, group 32, f16.  One process, the
arms alternating, HIP-graph replays timed with device events (eager launches where an arm does not capture), a warm-up per
shape, every window >= 0.2 s.  Run it twice to see the spread.
    PYTHONPATH=. timeout 900 python tools/wna16_g32_bench.py [out.txt] [M ...]"""
import os
import sys

import torch

from aphrodite_engine_amd import _custom_ops as ops

DEV = "cuda"
#         projection          K      N
SHAPES = [("8B qkv", 4096, 6144), ("8B o", 4096, 4096), ("8B gate_up", 4096, 28672), ("8B down", 14336, 4096),
          ("70B/TP8 o", 1024, 8192), ("70B/TP8 down", 3584, 8192)]
out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].isdigit() else None
Ms = [int(x) for x in sys.argv[1:] if x.isdigit()] or [65, 96, 128, 192, 256, 512, 1024, 2048, 4096, 8192]
ROUNDS, WINDOW_S, PEAK = 3, 0.2, 2.5e15


def graph_of(fn, iters):
    """-> a callable that runs fn iters times: a captured graph's replay, or (the arm does not capture) eager launches."""
    fn()
    torch.cuda.synchronize()
    try:
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for _ in range(iters):
                fn()
        gr.replay()
        torch.cuda.synchronize()
        return gr.replay, "graph"
    except RuntimeError:
        torch.cuda.synchronize()

        def eager():
            for _ in range(iters):
                fn()
        return eager, "eager"


def window(run, reps, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        run()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e-3 / (iters * reps)


lines = ["per call, microseconds from device events; new = wna16_gemm_large_g32(a[:, perm]), old = gptq_gemm(bit 4, exllama, perm) with "
         "APHRO_WNA16_NO_LARGE=1 (decode-kernel passes below 256 rows, gptq_dequant + torch.matmul from 256); TFLOP/s = 2 M N K / new; "
         "of peak = / 2.5 PFLOP/s (f16 dense MFMA), whole call incl. the gather; diff = max |new - old| / max |old|",
         f"{'projection':13s} {'K':>5s} {'N':>5s} {'M':>5s} {'new us (min..max)':>22s} {'old us (min..max)':>22s} {'old/new':>8s} "
         f"{'TFLOP/s':>8s} {'of peak':>8s} {'diff':>8s} {'timed as':>12s}"]
print("\n".join(lines), flush=True)
g = torch.Generator(device=DEV).manual_seed(0)


def old_call(a, qw, qz, sc, perm):
    os.environ["APHRO_WNA16_NO_LARGE"] = "1"
    try:
        return ops.gptq_gemm(a, qw, qz, sc, perm, True, 4)
    finally:
        del os.environ["APHRO_WNA16_NO_LARGE"]


for name, K, N in SHAPES:
    G = K // 32
    qw = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 8, N), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
    qz = torch.randint(-2 ** 31, 2 ** 31 - 1, (G, N // 8), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
    sc = (torch.rand(G, N, generator=g, device=DEV) * 0.01 + 0.005).half()
    perm = torch.randperm(K, generator=g, device=DEV).to(torch.int32)
    for M in Ms:
        iters = 20 if M <= 512 else 4
        a = torch.randn(M, K, generator=g, device=DEV).half()
        new = lambda: ops.wna16_gemm_large_g32(a[:, perm.long()], qw, qz, sc, 1)                  # noqa: E731
        old = lambda: old_call(a, qw, qz, sc, perm)                                               # noqa: E731
        y_old = old().float()
        diff = ((new().float() - y_old).abs().max() / y_old.abs().max()).item()
        del y_old
        (r_new, how_new), (r_old, how_old) = graph_of(new, iters), graph_of(old, iters)
        reps_new = max(1, int(WINDOW_S / (window(r_new, 2, iters) * iters)) + 1)
        reps_old = max(1, int(WINDOW_S / (window(r_old, 2, iters) * iters)) + 1)
        t_new, t_old = [], []
        for _ in range(ROUNDS):                    # alternate: drift of the box hits both alike
            t_new.append(window(r_new, reps_new, iters))
            t_old.append(window(r_old, reps_old, iters))
        del r_new, r_old
        tn, to = min(t_new), min(t_old)
        fl = 2.0 * M * N * K
        line = (f"{name:13s} {K:5d} {N:5d} {M:5d} {tn * 1e6:9.2f}..{max(t_new) * 1e6:<9.2f}   {to * 1e6:9.2f}..{max(t_old) * 1e6:<9.2f} "
                f"{to / tn:8.2f} {fl / tn / 1e12:8.1f} {fl / tn / PEAK:8.3f} {diff:8.1e} {how_new + '/' + how_old:>12s}")
        lines.append(line)
        print(line, flush=True)
        if out_path:                               # (kept current: a run cut short still leaves its rows)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")
