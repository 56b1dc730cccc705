"""One int4 sparse-MLP layer (fused_wna16_moe: routing, both expert GEMMs, combine) at prompt sizes: the prompt-sized grouped
kernel (csrc/moe_wna16_gemm_large.hip, large=True) against the decode-sized grouped path (large=False: moe_gather_pack + 16-row
m-tiles), and -- as context, not a bar -- the DENSE prompt kernel (ops._wna16_large) on gate_up + down at the same total rows
T topk.  Mixtral-8x7B shapes (E 8, top-2, H 4096, I 14336 and its TP-4 slice 3584), group 128, f16, uniform random routing.
One process, the arms alternating, HIP-graph replays timed with device events, a warm-up per shape, every window >= 0.2 s.
    PYTHONPATH=. timeout 900 python tools/moe_prefill_bench.py [out.txt] [T ...]
Kernel time of the new path alone, in a run of its own (the trace slows the host):
    PYTHONPATH=. rocprofv3 --kernel-trace --stats -d <dir> -- python tools/moe_prefill_bench.py --once <T> <I>
(three eager calls; per-kernel durations are the `kernels` view of the result database it writes)."""
import sys

import torch

from aphrodite_engine_amd import _custom_ops as ops
from aphrodite_engine_amd import moe as M

DEV = "cuda"
E, TOPK, H, GS = 8, 2, 4096, 128
INTERS = [14336, 3584]
ROUNDS, WINDOW_S = 3, 0.2
g = torch.Generator(device=DEV).manual_seed(0)


def rand_i32(*shape):
    return torch.randint(-2 ** 31, 2 ** 31 - 1, shape, generator=g, device=DEV, dtype=torch.int64).to(torch.int32)


def random_experts(inter):
    """Wna16Experts with random contents in the final layouts (every int32 is a valid word of nibbles in any order)."""
    ex = M.Wna16Experts.__new__(M.Wna16Experts)
    sc = lambda groups, n: (torch.rand(E, groups, n, generator=g, device=DEV) * 0.01 + 0.005).half()      # noqa: E731
    ex.w13 = (rand_i32(E, H // 8, 2 * inter), rand_i32(E, H // GS, 2 * inter // 8), sc(H // GS, 2 * inter))
    ex.w2 = (rand_i32(E, inter // 8, H), rand_i32(E, inter // GS, H // 8), sc(inter // GS, H))
    ex.zero_offset, ex.num_experts, ex.hidden, ex.inter = 1, E, H, inter
    return ex


def graph_of(fn, iters):
    fn()
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        for _ in range(iters):
            fn()
    gr.replay()
    torch.cuda.synchronize()
    return gr.replay


def window(run, reps, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        run()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) * 1e-3 / (iters * reps)


def inputs(t_):
    return torch.randn(t_, H, generator=g, device=DEV).half() * 0.5, torch.randn(t_, E, generator=g, device=DEV)


if len(sys.argv) > 1 and sys.argv[1] == "--once":
    t_, inter = int(sys.argv[2]), int(sys.argv[3])
    ex, (x, gate) = random_experts(inter), inputs(t_)
    for _ in range(3):
        M.fused_wna16_moe(x, ex, gate, TOPK, large=True)
    torch.cuda.synchronize()
    sys.exit(0)

out_path = sys.argv[1] if len(sys.argv) > 1 and not sys.argv[1].isdigit() else None
Ts = [int(v) for v in sys.argv[1:] if v.isdigit()] or [128, 256, 512, 1024, 2048, 4096, 8192]
lines = ["per sparse-MLP layer, microseconds from device events (graph replays); new = fused_wna16_moe(large=True), old = (large=False); "
         "rows/E = T topk / E; TFLOP/s = 2 T topk 3 H I / time; dense = ops._wna16_large gate_up + down at T topk rows (no routing, no "
         "SiluAndMul, no combine: context); diff = max |new - old| / max |old|",
         f"{'I':>6s} {'T':>5s} {'rows/E':>6s} {'new us (min..max)':>24s} {'old us (min..max)':>24s} {'old/new':>8s} {'new TF/s':>9s} "
         f"{'old TF/s':>9s} {'dense us':>10s} {'dense TF/s':>10s} {'diff':>8s}"]
print("\n".join(lines), flush=True)
for inter in INTERS:
    ex = random_experts(inter)
    dq13, dz13, ds13 = (v[0].contiguous() for v in ex.w13)
    dq2, dz2, ds2 = (v[0].contiguous() for v in ex.w2)
    for t_ in Ts:
        iters = 8 if t_ <= 1024 else 2
        x, gate = inputs(t_)
        new = lambda: M.fused_wna16_moe(x, ex, gate, TOPK, large=True)                            # noqa: E731
        old = lambda: M.fused_wna16_moe(x, ex, gate, TOPK, large=False)                           # noqa: E731
        xd = torch.randn(t_ * TOPK, H, generator=g, device=DEV).half() * 0.5
        ad = torch.randn(t_ * TOPK, inter, generator=g, device=DEV).half() * 0.5
        dense = lambda: (ops._wna16_large(xd, dq13, dz13, ds13, None, 1), ops._wna16_large(ad, dq2, dz2, ds2, None, 1))   # noqa: E731
        y_old = old().float()
        diff = ((new().float() - y_old).abs().max() / y_old.abs().max()).item()
        del y_old
        r_new, r_old, r_dense = graph_of(new, iters), graph_of(old, iters), graph_of(dense, iters)
        reps = [max(1, int(WINDOW_S / (window(r, 2, iters) * iters)) + 1) for r in (r_new, r_old, r_dense)]
        t_new, t_old, t_dense = [], [], []
        for _ in range(ROUNDS):                    # alternate: drift of the box hits every arm alike
            t_new.append(window(r_new, reps[0], iters))
            t_old.append(window(r_old, reps[1], iters))
            t_dense.append(window(r_dense, reps[2], iters))
        del r_new, r_old, r_dense
        tn, to, td = min(t_new), min(t_old), min(t_dense)
        fl = 2.0 * t_ * TOPK * 3 * H * inter
        line = (f"{inter:6d} {t_:5d} {t_ * TOPK // E:6d} {tn * 1e6:10.1f}..{max(t_new) * 1e6:<10.1f}   {to * 1e6:10.1f}..{max(t_old) * 1e6:<10.1f} "
                f"{to / tn:8.2f} {fl / tn / 1e12:9.1f} {fl / to / 1e12:9.1f} {td * 1e6:10.1f} {fl / td / 1e12:10.1f} {diff:8.1e}")
        lines.append(line)
        print(line, flush=True)
        if out_path:                               # (kept current: a run cut short still leaves its rows)
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")
