"""Prompt-sized 8-bit GPTQ GEMM (csrc/gptq8_gemm_large.hip, ops.gptq8_gemm_large) against the path it replaces
(ops.gptq_dequant(..., 8) + torch.matmul on the same tensors) on the Llama-3-8B projections at 8 bits, group 128, and one
channel-wise shape; for context the 4-bit kernel (ops.gptq_gemm, bit 4) at the same (M, N, K).  f16.  One process, the
paths alternating, HIP-graph replays timed with device events, every window >= 0.3 s.  Run it twice to see the spread.
    PYTHONPATH=. timeout 900 python tools/gptq8_large_bench.py [out.txt] [M ...]"""
import sys

import torch

from aphrodite_engine_amd import _custom_ops as ops

DEV = "cuda"
#         projection        K      N      G
SHAPES = [("qkv", 4096, 6144, 32), ("o", 4096, 4096, 32), ("gate_up", 4096, 28672, 32), ("down", 14336, 4096, 112),
          ("o channel-wise", 4096, 4096, 1)]
out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].isdigit() else None
Ms = [int(x) for x in sys.argv[1:] if x.isdigit()] or [65, 128, 256, 512, 1024, 2048, 8192]
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


lines = ["per call, microseconds from device events around graph replays; new = gptq8_gemm_large, old = gptq_dequant(8) + torch.matmul, "
         "w4 = the 4-bit prompt kernel at the same (M, N, K), eager launches (host-bound where it is short); TFLOP/s = 2 M N K / new; of peak = / 2.5 PFLOP/s (f16 dense); "
         "diff = max |new - old| / max |old|",
         f"{'projection':15s} {'K':>5s} {'N':>5s} {'G':>4s} {'M':>5s} {'new us (min..max)':>22s} {'old us (min..max)':>22s} {'old/new':>8s} "
         f"{'TFLOP/s':>8s} {'of peak':>8s} {'w4 us':>9s} {'diff':>8s}"]
print("\n".join(lines), flush=True)
g = torch.Generator(device=DEV).manual_seed(0)
empty = torch.empty(0, dtype=torch.int32, device=DEV)


def rand_words(shape):
    return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, device=DEV, dtype=torch.int64).to(torch.int32)


for name, K, N, G in SHAPES:
    qw, qz, qw4, qz4 = rand_words((K // 4, N)), rand_words((G, N // 4)), rand_words((K // 8, N)), rand_words((G, N // 8))
    sc = (torch.rand(G, N, generator=g, device=DEV) * 0.01 + 0.005).half()
    for M in Ms:
        iters = 20 if M <= 512 else 4
        a = torch.randn(M, K, generator=g, device=DEV).half()
        new = lambda: ops.gptq8_gemm_large(a, qw, qz, sc)                                         # noqa: E731
        old = lambda: torch.matmul(a, ops.gptq_dequant(qw, qz, sc, empty, True, 8))                # noqa: E731
        w4 = lambda: ops.gptq_gemm(a, qw4, qz4, sc, empty, True, 4)                                # noqa: E731
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
        del g_old
        t4 = "-"
        if ops.wna16_large_ok(M, N, K, G):          # (eager launches: its large plans clear flags with a memset node)
            w4()
            torch.cuda.synchronize()
            s4, e4 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            n4 = max(20, int(WINDOW_S / min(t_new)) // 2)
            s4.record()
            for _ in range(n4):
                w4()
            e4.record()
            e4.synchronize()
            t4 = f"{s4.elapsed_time(e4) * 1e3 / n4:9.2f}"
        tn, to = min(t_new), min(t_old)
        fl = 2.0 * M * N * K
        line = (f"{name:15s} {K:5d} {N:5d} {G:4d} {M:5d} {tn * 1e6:9.2f}..{max(t_new) * 1e6:<9.2f}   {to * 1e6:9.2f}..{max(t_old) * 1e6:<9.2f} "
                f"{to / tn:8.2f} {fl / tn / 1e12:8.1f} {fl / tn / PEAK:8.3f} {t4:>9s} {diff:8.1e}")
        lines.append(line)
        print(line, flush=True)
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
