"""Checkpoint-order GPTQ decode GEMM (csrc/gptq_gidx_gemm.hip, ops.gptq_gemm_gidx; above 32 rows in 32-row passes) against
the path it replaces (ops.gptq_dequant + torch.matmul on the same tensors), on the row-parallel projections of a TP shard:
f16, act-order g_idx, scales / zeros of the unsharded matrix.  One process, the two paths alternating, HIP-graph replays
timed with device events, every window >= 0.3 s.  Run it twice to see the spread.
    timeout 600 python tools/gptq_gidx_bench.py [out.txt] [M ...]"""
import sys

import torch

from aphrodite_engine_amd import _custom_ops as ops

DEV = "cuda"
#         shard                        K     N     G (groups of the unsharded matrix, 128 rows each)
SHAPES = [("70B down_proj TP8", 3584, 8192, 224), ("70B o_proj TP8", 1024, 8192, 64), ("Llama-3-8B down_proj TP2", 7168, 4096, 112)]
out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].isdigit() else None
Ms = [int(x) for x in sys.argv[1:] if x.isdigit()] or [1, 8, 32, 64, 128]
ITERS, ROUNDS, WINDOW_S = 20, 3, 0.3


def graph_of(fn):
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(ITERS):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    return gr


def window(gr, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        gr.replay()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e-3 / (ITERS * reps)


lines = ["per call, seconds from device events around graph replays; new = gptq_gemm_gidx kernel (32-row passes), old = gptq_dequant + "
         "torch.matmul; bytes = K*N/2 + activations + scale/zero table + output (algorithmic, not measured); share = bytes / time / 8 TB/s",
         f"{'shard':26s} {'K':>5s} {'N':>5s} {'G':>4s} {'M':>4s} {'new us (min..max)':>22s} {'old us (min..max)':>22s} {'old/new':>8s} "
         f"{'alg MB':>7s} {'alg GB/s':>9s} {'of 8 TB/s':>9s} {'max err':>8s}"]
print("\n".join(lines), flush=True)
g = torch.Generator(device=DEV).manual_seed(0)
for name, K, N, G in SHAPES:
    qw = torch.randint(-2 ** 31, 2 ** 31 - 1, (K // 8, N), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
    qz = torch.randint(-2 ** 31, 2 ** 31 - 1, (G, N // 8), generator=g, device=DEV, dtype=torch.int64).to(torch.int32)
    sc = (torch.rand(G, N, generator=g, device=DEV) * 0.01 + 0.005).half()
    g_idx = (torch.randperm(G * 128, generator=g, device=DEV)[:K] // 128).to(torch.int32)
    for M in Ms:
        a = torch.randn(M, K, generator=g, device=DEV).half()
        new = lambda: ops.gptq_gemm_gidx(a, qw, qz, sc, g_idx, 1)                                  # noqa: E731
        old = lambda: torch.matmul(a, ops.gptq_dequant(qw, qz, sc, g_idx, False, 4))               # noqa: E731
        ref = a.double() @ ops.gptq_dequant(qw, qz, sc, g_idx, False, 4).double()
        err = ((new().double() - ref).abs().max() / ref.abs().max()).item()
        g_new, g_old = graph_of(new), graph_of(old)
        reps_new = max(1, int(WINDOW_S / (window(g_new, 2) * ITERS)) + 1)
        reps_old = max(1, int(WINDOW_S / (window(g_old, 2) * ITERS)) + 1)
        t_new, t_old = [], []
        for _ in range(ROUNDS):                    # alternate: drift of the box hits both alike
            t_new.append(window(g_new, reps_new))
            t_old.append(window(g_old, reps_old))
        by = K * N / 2 + M * K * 2 + G * N * 2.5 + K * 4 + M * N * 2
        tn, to = min(t_new), min(t_old)
        line = (f"{name:26s} {K:5d} {N:5d} {G:4d} {M:4d} {tn * 1e6:9.2f}..{max(t_new) * 1e6:<9.2f}   {to * 1e6:9.2f}..{max(t_old) * 1e6:<9.2f} "
                f"{to / tn:8.2f} {by / 1e6:7.2f} {by / tn / 1e9:9.0f} {by / tn / 8e12:9.3f} {err:8.1e}")
        lines.append(line)
        print(line, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
