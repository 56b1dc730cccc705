#!/usr/bin/env python3
"""Attention logit soft cap against the uncapped kernels on identical inputs, us per launch (device events; capped and
uncapped alternate round by round; median and min..max over the rounds).

decode : bs 32 at context 1024 / 8192, head 128 (32 q / 8 kv heads) and head 256 (16 / 8), v1 form inside a HIP graph with the
         KV cold (six caches cycled); plus bs 4 at context 8192, head 128, where the launcher splits the KV over workgroups
         (the split form has the capped variant too).
prefill: one sequence of T = 2048 / 8192, head 128 (32 / 8) without and with a 4096 window, head 256 (16 / 8).  A capped head-128
         call without a window runs on the second-generation kernel while the uncapped one goes to the third / fourth; `v2`
         rows pin the uncapped call to the second generation with a window that covers every key (its mask arithmetic then
         runs on every tile, for both sides of that row).  `capped v2 | capped v4` rows: the capped call on the second generation
         (APHRO_FA_V4_MIN_KEYS huge) against the capped fourth generation (APHRO_FA_V4_MIN_KEYS=1024), T = 1100 / 2048 / 4096 / 8192."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aphrodite_engine_amd import _custom_ops as ops  # noqa: E402

dev, CAP, ROUNDS = "cuda", 50.0, 7
g = torch.Generator(device=dev).manual_seed(0)


def timed(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e3 / reps


def compare(label, plain, capped, reps, per_call=1, names=("uncapped", "capped")):
    """plain / capped: callables of the same work; alternating rounds"""
    for fn in (plain, capped):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(ROUNDS):
        a.append(timed(plain, reps) / per_call)
        b.append(timed(capped, reps) / per_call)
    ma, mb = statistics.median(a), statistics.median(b)
    print(f"{label:<58} {names[0]:<8} {ma:9.1f} us ({min(a):.1f}..{max(a):.1f})   {names[1]:<6} {mb:9.1f} us ({min(b):.1f}..{max(b):.1f})"
          f"   +{mb - ma:8.1f} us  x{mb / ma:.3f}", flush=True)


def decode(B, H, HKV, HD, ctx, BS=16, NC=6):
    nblk = (ctx + BS - 1) // BS
    caches = [((torch.randn(B * nblk, HKV, HD // 8, BS, 8, device=dev, generator=g) * 0.5).half(),
               (torch.randn(B * nblk, HKV, HD, BS, device=dev, generator=g) * 0.5).half()) for _ in range(NC)]
    bt = torch.randperm(B * nblk, device=dev, generator=g).to(torch.int32).view(B, nblk).contiguous()
    seq_lens = torch.full((B, ), ctx, dtype=torch.int32, device=dev)
    q = (torch.randn(B, H, HD, device=dev, generator=g) * 4).half()
    o = torch.empty_like(q)
    graphs = []
    for cap in (0.0, CAP):
        def launches():
            for kc, vc in caches:
                ops.paged_attention_v1(o, q, kc, vc, HKV, HD ** -0.5, bt, seq_lens, BS, ctx, None, "auto", 1.0, 1.0, softcap=cap)
        launches()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            launches()
        graphs.append(gr)
    compare(f"decode  bs {B:<3} ctx {ctx:<5} head {HD} ({H}/{HKV})", graphs[0].replay, graphs[1].replay, 20, per_call=NC)


def prefill(T, H, HKV, HD, window, pin_v2=False):
    qkv = (torch.randn(T, (H + 2 * HKV) * HD, device=dev, generator=g) * 2).half()
    q, k, v = qkv.split([H * HD, HKV * HD, HKV * HD], dim=-1)
    q, k, v = q.view(T, H, HD), k.view(T, HKV, HD), v.view(T, HKV, HD)
    cu = torch.tensor([0, T], dtype=torch.int32, device=dev)
    w = (T, T) if pin_v2 else ((window, window) if window else None)
    run = lambda cap: ops.flash_attn_varlen(q, k, v, cu, T, HD ** -0.5, causal=True, window_size=w, softcap=cap)
    tag = "v2 (window >= T)" if pin_v2 else (f"window {window}" if window else "no window")
    compare(f"prefill T {T:<5} head {HD} ({H}/{HKV}) {tag}", lambda: run(0.0), lambda: run(CAP), 20 if T <= 2048 else 5)


def capped_v2_v4(T, H=32, HKV=8, HD=128):
    qkv = (torch.randn(T, (H + 2 * HKV) * HD, device=dev, generator=g) * 2).half()
    q, k, v = qkv.split([H * HD, HKV * HD, HKV * HD], dim=-1)
    q, k, v = q.view(T, H, HD), k.view(T, HKV, HD), v.view(T, HKV, HD)
    cu = torch.tensor([0, T], dtype=torch.int32, device=dev)

    cur = [None]

    def run(min_keys):      # (the knob is switched only when it changes: once per timed round, outside the event pair's work)
        if cur[0] != min_keys:
            os.environ["APHRO_FA_V4_MIN_KEYS"] = str(min_keys)
            ops.reload_env()
            cur[0] = min_keys
        return ops.flash_attn_varlen(q, k, v, cu, T, HD ** -0.5, causal=True, softcap=CAP)
    err = (run(1 << 30).float() - run(1024).float()).abs().max().item()
    print(f"prefill T {T:<5} head {HD} ({H}/{HKV}) capped v2 | capped v4: max |difference| {err:.2e}")
    compare(f"prefill T {T:<5} head {HD} ({H}/{HKV}) capped v2 | capped v4", lambda: run(1 << 30), lambda: run(1024), 20 if T <= 2048 else 5,
            names=("v2", "v4"))
    os.environ.pop("APHRO_FA_V4_MIN_KEYS")
    ops.reload_env()


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the MI355X"
    for hd, h, hkv in ((128, 32, 8), (256, 16, 8)):
        for ctx in (1024, 8192):
            decode(32, h, hkv, hd, ctx)
    decode(4, 32, 8, 128, 8192)
    for T in (2048, 8192):
        prefill(T, 32, 8, 128, 0)
        prefill(T, 32, 8, 128, 0, pin_v2=True)
        prefill(T, 32, 8, 128, 4096)
        prefill(T, 16, 8, 256, 0)
    for T in (1100, 2048, 4096, 8192):
        capped_v2_v4(T)
