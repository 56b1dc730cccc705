"""Prompt-sized checkpoint-order GPTQ GEMM (csrc/gptq_gidx_gemm_large.hip, ops.gptq_gemm_gidx_large) against the path it
replaces (ops.gptq_dequant(..., g_idx, False, 4) + torch.matmul on the same tensors) on the row-parallel projections of
Llama-3-8B at TP 2 and of a 70B at TP 8, group 128, random act-order g_idx over the UNSHARDED group count.  f16.  One
process, the paths alternating, HIP-graph replays timed with device events, every window >= 0.3 s.  Run it twice to see the
spread.
    PYTHONPATH=. timeout 900 python tools/gptq_gidx_large_bench.py [out.txt] [M ...]"""
import sys

import torch

from aphrodite_engine_amd import _custom_ops as ops

DEV = "cuda"
#         projection            K      N      G
SHAPES = [("8B o, TP2", 2048, 4096, 32), ("8B down, TP2", 7168, 4096, 112), ("70B o, TP8", 1024, 8192, 64),
          ("70B down, TP8", 3584, 8192, 224)]
out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].isdigit() else None
Ms = [int(x) for x in sys.argv[1:] if x.isdigit()] or [65, 96, 128, 129, 136, 144, 152, 160, 176, 192, 224, 256, 512, 1024, 2048, 4096, 8192]
ROUNDS, WINDOW_S, PEAK = 3, 0.3, 2.5e15


def graph_of(fn, iters):
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(iters):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    return gr


def window(gr, reps, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        gr.replay()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e-3 / (iters * reps)


lines = ["per call, microseconds from device events around graph replays; new = gptq_gemm_gidx_large, old = gptq_dequant(g_idx) + torch.matmul; "
         "TFLOP/s = 2 M N K / new; of peak = / 2.5 PFLOP/s (f16 dense); diff = max |new - old| / max |old|",
         f"{'projection':15s} {'K':>5s} {'N':>5s} {'G':>4s} {'M':>5s} {'new us (min..max)':>22s} {'old us (min..max)':>22s} {'old/new':>8s} "
         f"{'TFLOP/s':>8s} {'of peak':>8s} {'diff':>8s}"]
print("\n".join(lines), flush=True)
g = torch.Generator(device=DEV).manual_seed(0)

for name, K, N, G in SHAPES:
    qw = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 8, N), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
    qz = torch.randint(-2 ** 31, 2 ** 31 - 1, (G, N // 8), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
    sc = (torch.rand(G, N, generator=g, device=DEV) * 0.01 + 0.005).half()
    g_idx = torch.randint(0, G, (K,), generator=g, device=DEV, dtype=torch.int32)
    for M in Ms:
        iters = 20 if M <= 512 else 4
        a = torch.randn(M, K, generator=g, device=DEV).half()
        new = lambda: ops.gptq_gemm_gidx_large(a, qw, qz, sc, g_idx, 1)                            # noqa: E731
        old = lambda: torch.matmul(a, ops.gptq_dequant(qw, qz, sc, g_idx, False, 4))               # noqa: E731
        y_old = old().float()
        diff = ((new().float() - y_old).abs().max() / y_old.abs().max()).item()
        del y_old
        g_new, g_old = graph_of(new, iters), graph_of(old, iters)
        reps_new = max(1, int(WINDOW_S / (window(g_new, 2, iters) * iters)) + 1)
        reps_old = max(1, int(WINDOW_S / (window(g_old, 2, iters) * iters)) + 1)
        t_new, t_old = [], []
        for _ in range(ROUNDS):                    # alternate: drift of the box hits both alike
            t_new.append(window(g_new, reps_new, iters))
            t_old.append(window(g_old, reps_old, iters))
        del g_new, g_old
        tn, to = min(t_new), min(t_old)
        fl = 2.0 * M * N * K
        line = (f"{name:15s} {K:5d} {N:5d} {G:4d} {M:5d} {tn * 1e6:9.2f}..{max(t_new) * 1e6:<9.2f}   {to * 1e6:9.2f}..{max(t_old) * 1e6:<9.2f} "
                f"{to / tn:8.2f} {fl / tn / 1e12:8.1f} {fl / tn / PEAK:8.3f} {diff:8.1e}")
        lines.append(line)
        print(line, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
