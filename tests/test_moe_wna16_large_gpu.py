"""The prompt-sized grouped W4A16 GEMM of the sparse MLP (csrc/moe_wna16_gemm_large.hip) against the fp64 oracle:
ops.wna16_gemm_grouped_large in its three epilogues, fused_wna16_moe on the new path, HIP-graph replay.  Rows per expert
130 / 0 / 128 / 62 at block 128: a full tile + a 2-row tail, an expert without rows, an exact tile, a partial tile; padding rows
in three of the four active tiles, three tiles past the padded count."""
import functools

import numpy as np
import pytest
import torch

from oracle import attention as oa
from oracle import moe as om
from oracle import quant as oq

pytestmark = pytest.mark.gpu
DEV = "cuda"
E, GS, TOPK = 4, 128, 2
ROWS = (130, 0, 128, 62)
#         K     N    bn (0: planned)
CASES = [(128, 128, 0),          # one K-tile pair: pipeline prologue and epilogue only
         (384, 256, 0),          # odd number of K-tile pairs, a group boundary every second tile
         (384, 256, 256),        # the same on the 4-wave 256-column tile
         (1024, 384, 0)]         # three column tiles
DTYPES = [torch.float16, torch.bfloat16]
TOL = {torch.float16: 3e-3, torch.bfloat16: 1.6e-2}        # tests/test_wna16_g32_large_gpu.py: the same arithmetic
TOL_MLP = {torch.float16: 4e-3, torch.bfloat16: 3e-2}      # test_fused_wna16_moe's


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a visible MI355X (torch.cuda.is_available() is False)")
    from aphrodite_engine_amd import _custom_ops, _lib
    _lib.lib()
    return _custom_ops


def dev(x, dtype=None):
    x = torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    return x if dtype is None else x.to(dtype)


@functools.lru_cache(maxsize=None)
def weights(k, n, exact, dtype, seed=0):
    """E experts -> per-expert checkpoint-order sets (qweight [K/8, N], stored zeros [G, N/8], scales [G, N] in dtype) on the
    device, and their fp64 dequantisation [E, K, N] on the dtype-rounded scales."""
    rng = np.random.default_rng(k + n + exact + seed)
    sets, w64 = [], []
    for _ in range(E):
        q = rng.integers(0, 16, size=(k, n))
        z = rng.integers(0, 16, size=(k // GS, n))
        q[0, 0], q[1, 0], z[0, 0], z[0, 1] = 0, 15, 0, 15            # stored zero 15 means 16
        s = 2.0 ** -rng.integers(6, 10, size=(k // GS, n)) if exact else rng.uniform(0.002, 0.02, size=(k // GS, n))
        s_t = dev(s.astype(np.float32), dtype)
        sets.append((dev(oq.gptq_pack(q, 4)), dev(oq.pack_cols(z, 4)), s_t))
        w64.append(oq.gptq_dequant(oq.gptq_pack(q, 4), oq.pack_cols(z, 4), s_t.float().cpu().numpy()).astype(np.float64))
    return sets, np.stack(w64)


def grouped_case(ops, k, n, exact, dtype, mode, bn=0, zero_offset=1):
    """The op on the crafted routing -> (its non-padding rows, the fp64 oracle rows a[slot // topk] . W[expert of slot])."""
    sets, w64 = weights(k, n, exact, dtype)
    rng = np.random.default_rng(k)
    topk_ids = rng.permutation(np.repeat(np.arange(E), ROWS)).reshape(-1, TOPK).astype(np.int32)
    sorted_ids, expert_ids, post = om.moe_align_block_size(topk_ids, E, 128)
    t_ = topk_ids.shape[0]
    a = rng.integers(-2, 3, size=(t_, k)).astype(np.float32) if exact else (rng.standard_normal((t_, k)) * 0.5).astype(np.float32)
    a = dev(a, dtype)
    qw = torch.stack([dev(oq.gptq_shuffle(s[0].cpu().numpy())) for s in sets])
    qz = torch.stack([s[1] for s in sets])
    if zero_offset == 0:        # the AWQ form: the stored nibble IS the zero point -> every weight one scale above GPTQ's reading
        w64 = w64 + np.stack([np.repeat(s[2].double().cpu().numpy(), GS, axis=0) for s in sets])
    got = ops.wna16_gemm_grouped_large(a, dev(sorted_ids), TOPK, qw, qz, torch.stack([s[2] for s in sets]), dev(expert_ids),
                                       dev(np.array([post], np.int32)), zero_offset, mode, bn=bn)
    got = got[0] if mode == "slab" else got
    rows = np.nonzero(sorted_ids[:post] < topk_ids.size)[0]
    slots = sorted_ids[rows]
    a64 = a.double().cpu().numpy()
    ref = np.stack([a64[s // TOPK] @ w64[topk_ids.reshape(-1)[s]] for s in slots])
    return got[dev(rows).long()], ref


def close(got, ref, tol):
    got = got.float().cpu().numpy()
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=tol, atol=tol * np.abs(ref).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,n,bn", CASES)
def test_moe_wna16_large_exact(ops, k, n, bn, dtype):
    """Bit equality on inputs whose every product and partial sum is exact in fp32: a wrong gathered row, another expert's
    weights, the neighbouring group's zero point or a misplaced nibble cannot hide under a tolerance."""
    assert k * 2 * 16 * 2 ** 3 <= 2 ** 23
    got, ref = grouped_case(ops, k, n, True, dtype, "out", bn)
    assert torch.equal(got.cpu(), torch.from_numpy(ref).to(dtype))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k,n,bn", CASES[1:])
def test_moe_wna16_large_vs_oracle(ops, k, n, bn, dtype):
    got, ref = grouped_case(ops, k, n, False, dtype, "out", bn)
    close(got, ref, TOL[dtype])
    got, ref = grouped_case(ops, k, n, False, dtype, "silu", bn)     # columns 2j = gate_j, 2j + 1 = up_j
    close(got, oa.silu_and_mul(np.concatenate([ref[:, 0::2], ref[:, 1::2]], axis=1)), TOL_MLP[dtype])
    got, ref = grouped_case(ops, k, n, False, dtype, "slab", bn)
    close(got, ref, TOL[torch.float16])                             # fp32, unrounded: the f16 rounding of the weights alone


def test_moe_wna16_large_zero_offset_0(ops):
    got, ref = grouped_case(ops, 384, 256, False, torch.float16, "out", zero_offset=0)
    close(got, ref, TOL[torch.float16])


def layer_case(ops, t_, dtype, h=256):
    from aphrodite_engine_amd import moe as M
    i = h
    s13, w13 = weights(h, 2 * i, False, dtype, 1)
    s2, w2 = weights(i, h, False, dtype, 2)
    rng = np.random.default_rng(t_)
    x = dev((rng.standard_normal((t_, h)) * 0.5).astype(np.float32), dtype)
    gating = dev(rng.standard_normal((t_, E)).astype(np.float32))
    return M, M.Wna16Experts(list(s13), list(s2)), x, gating, w13, w2


@pytest.mark.parametrize("dtype", DTYPES)
def test_moe_wna16_large_layer(ops, dtype):
    t_ = ops.MOE_WNA16_LARGE_MIN_ROWS * E // TOPK + 3                # the committed threshold: the new path is what runs
    M, experts, x, gating, w13, w2 = layer_case(ops, t_, dtype)
    m_pad = (t_ * TOPK + E * 127 + 127) // 128 * 128
    assert ops.moe_wna16_large_ok(m_pad, 512, 256, 2, E, dtype) and ops.moe_wna16_large_ok(m_pad, 256, 256, 2, E, dtype)
    assert M.moe_large_routed(t_, TOPK, experts, dtype) and not M.moe_large_routed(33, TOPK, experts, dtype)
    got = M.fused_wna16_moe(x, experts, gating, TOPK, renormalize=True).float().cpu().numpy()
    rw, rids, _ = om.topk_softmax(gating.cpu().numpy(), TOPK)
    ref = om.moe_layer(x.float().cpu().numpy(), w13, w2, rw / rw.sum(axis=1, keepdims=True), rids)
    assert np.abs(got - ref).mean() / np.abs(ref).mean() < 0.04
    np.testing.assert_allclose(got, ref, rtol=TOL_MLP[dtype], atol=TOL_MLP[dtype] * np.abs(ref).max())


def test_moe_wna16_large_below_threshold_untouched(ops):
    """Below the threshold the decode-sized path runs, bit for bit (H = I = 512: the smallest K its kernel serves)."""
    M, experts, x, gating, _, _ = layer_case(ops, 33, torch.float16, 512)
    assert not M.moe_large_routed(33, TOPK, experts, torch.float16)
    assert torch.equal(M.fused_wna16_moe(x, experts, gating, TOPK), M.fused_wna16_moe(x, experts, gating, TOPK, large=False))


def test_moe_wna16_large_graph_replay(ops):
    """Captured once, replayed with other activations AND routings of the same T (tile skipping and the gather read device
    memory only): every replay equals the eager call."""
    t_ = ops.MOE_WNA16_LARGE_MIN_ROWS * E // TOPK + 3
    M, experts, x, gating, _, _ = layer_case(ops, t_, torch.float16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        M.fused_wna16_moe(x, experts, gating, TOPK)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = M.fused_wna16_moe(x, experts, gating, TOPK)
    for seed in range(1, 4):
        gen = torch.Generator().manual_seed(seed)
        x.copy_((torch.randn(x.shape, generator=gen) * 0.5).to(DEV))
        gating.copy_(torch.randn(gating.shape, generator=gen).to(DEV))
        gating[:, seed] += 2.0                                       # a different load per expert each time
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, M.fused_wna16_moe(x, experts, gating, TOPK))
