"""The prompt-sized group-size-32 W4A16 GEMM (csrc/wna16_gemm_large_g32.hip) against the fp64 oracle, through every entry that
reaches it: ops.wna16_gemm_large_g32, the routing of ops.gptq_gemm / ops._wna16, HIP-graph replay, the C++ registration, the
layer.  Plans at the rows used here (65 / 129 / 200 / 256): a, b, c run one K slice; d eight (the split-K form: fp32 slabs + reduce)."""
import functools

import numpy as np
import pytest
import torch

from oracle import quant as oq

pytestmark = pytest.mark.gpu
DEV = "cuda"
GS = 32
#        K     N
CASES = {"a": (64, 128),         # one K tile (pipeline prologue and epilogue only); the group boundary inside the tile
         "b": (192, 384),        # odd number of K tiles, three column tiles
         "c": (1024, 256),       # act-order through perm
         "d": (4096, 128)}       # split-K at small M
TOL = {torch.float16: 3e-3, torch.bfloat16: 1.6e-2}      # tests/test_gptq_gidx_gpu.py: one rounding per weight and output, fp32 sums


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
def _weights(name, exact, n=None, gs=GS):
    """-> (qweight [K/8, N] in exllama order, on the device and as the oracle reads it; stored zeros [G, N] (zero - 1);
    scales fp32; perm)."""
    from aphrodite_engine_amd import _custom_ops as ops
    k, n_case = CASES[name]
    n = n or n_case
    rng = np.random.default_rng(ord(name) + n + exact + gs)
    q = rng.integers(0, 16, size=(k, n))
    z = rng.integers(0, 16, size=(k // gs, n))
    q[0, 0], q[1, 0], z[0, 0], z[0, 1] = 0, 15, 0, 15            # stored zero 15 means 16
    s = 2.0 ** -rng.integers(6, 10, size=(k // gs, n)) if exact else rng.uniform(0.002, 0.02, size=(k // gs, n))
    qw = dev(oq.gptq_pack(q, 4))
    ops.gptq_shuffle(qw, None, 4)
    return qw, qw.cpu().numpy(), z, s.astype(np.float32), rng.permutation(k).astype(np.int32)


def exact_case(name, m, dtype):
    """Inputs on which every product and every partial sum is exact in fp32 in any order (see the assert) -> device
    (a, qweight, qzeros, scales, 1) and the fp64 oracle result rounded once to dtype."""
    qw, qw_np, z, s, _ = _weights(name, True)
    k, amax = CASES[name][0], 1 if name == "d" else 2
    assert k * amax * 16 * 2 ** 3 <= 2 ** 23
    a = np.random.default_rng(m).integers(-amax, amax + 1, size=(m, k)).astype(np.float32)
    ref = torch.from_numpy(oq.gptq_gemm(a, qw_np, oq.pack_cols(z, 4), s, None, True, 4)).to(dtype)
    return [dev(a, dtype), qw, dev(oq.pack_cols(z, 4)), dev(s, dtype), 1], ref


def real_case(name, m, dtype, n=None, gs=GS):
    """-> device (a, qweight, qzeros, scales, perm), fp64 oracle result on the rounded a / scales (act-order through perm)."""
    qw, qw_np, z, s, perm = _weights(name, False, n, gs)
    a = dev((np.random.default_rng(m).standard_normal((m, CASES[name][0])) * 0.5).astype(np.float32), dtype)
    s_t = dev(s, dtype)
    ref = oq.gptq_gemm(a.float().cpu().numpy(), qw_np, oq.pack_cols(z, 4), s_t.float().cpu().numpy(), perm, True, 4)
    return (a, qw, dev(oq.pack_cols(z, 4)), s_t, dev(perm)), ref


def close(got, ref, dtype):
    got = got.float().cpu().numpy()
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=TOL[dtype], atol=TOL[dtype] * np.abs(ref).max())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("m", [65, 129])
@pytest.mark.parametrize("name", list(CASES))
def test_wna16_g32_exact(ops, name, m, dtype):
    """Bit equality: an off-by-one zero point, the first group's constants on the second half of a K tile or a misplaced
    nibble cannot hide under a tolerance here."""
    from aphrodite_engine_amd import _lib
    k, n = CASES[name]
    assert ops.wna16_large_g32_ok(m, n, k, k // GS, dtype)
    if name == "d":      # f16: the workspace is the fp32 slabs alone -> the split form is what runs
        assert _lib.lib().aphro_wna16_gemm_large_g32_workspace_bytes(m, n, k, k // GS, _lib.F16) == 8 * m * n * 4
    args, ref = exact_case(name, m, dtype)
    assert torch.equal(ops.wna16_gemm_large_g32(*args).cpu(), ref)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("m", [129, 256])
@pytest.mark.parametrize("name", ["b", "c"])
def test_wna16_g32_vs_oracle(ops, name, m, dtype):
    (a, qw, qz, s, perm), ref = real_case(name, m, dtype)
    close(ops.wna16_gemm_large_g32(a[:, perm.long()], qw, qz, s, 1), ref, dtype)


def test_wna16_g32_zero_offset_0(ops):
    """The AWQ-repacked / compressed-tensors form: the stored nibble IS the zero point (the oracle adds GPTQ's 1)."""
    (a, qw, _, s, perm), _ = real_case("b", 129, torch.float16)
    z = np.random.default_rng(7).integers(0, 15, size=(CASES["b"][0] // GS, CASES["b"][1]))
    ref = oq.gptq_gemm(a.float().cpu().numpy(), qw.cpu().numpy(), oq.pack_cols(z, 4), s.float().cpu().numpy(), None, True, 4)
    close(ops.wna16_gemm_large_g32(a, qw, dev(oq.pack_cols(z + 1, 4)), s, 0), ref, torch.float16)


def test_wna16_g32_routing(ops):
    m = 200                                                        # inside the measured window, a partial last m-block
    assert ops.WNA16_G32_LARGE_MIN_M <= m <= ops.WNA16_G32_LARGE_MAX_M
    (a, qw, qz, s, perm), ref = real_case("c", m, torch.float16)
    out = ops.gptq_gemm(a, qw, qz, s, perm, True, 4)
    assert torch.equal(out, ops.wna16_gemm_large_g32(a[:, perm.long()], qw, qz, s, 1))
    close(out, ref, torch.float16)


def test_wna16_g32_routing_untiled_n(ops):
    args96, ref96 = real_case("c", 200, torch.float16, n=96)      # no 128-column tiling: the decode kernel's passes
    assert not ops.wna16_large_g32_ok(200, 96, 1024, 1024 // GS, torch.float16)
    close(ops.gptq_gemm(*args96, True, 4), ref96, torch.float16)


def test_wna16_g32_routing_group_64_stays(ops):
    (a, qw, qz, s, perm), ref = real_case("c", 129, torch.float16, gs=64)
    assert not ops.wna16_large_g32_ok(129, 256, 1024, 1024 // 64, torch.float16)
    out = ops.gptq_gemm(a, qw, qz, s, perm, True, 4)
    assert torch.equal(out, ops._wna16_large(a, qw, qz, s, perm, 1))
    close(out, ref, torch.float16)


def test_wna16_g32_graph_replay(ops):
    """The split-K form (case d) captured once: every replay equals the eager call on the same activations."""
    args, _ = exact_case("d", 65, torch.float16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.wna16_gemm_large_g32(*args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.wna16_gemm_large_g32(*args)
    for seed in range(3):
        args[0].copy_(torch.randn(args[0].shape, generator=torch.Generator().manual_seed(seed)).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.wna16_gemm_large_g32(*args))


def test_wna16_g32_cpp_op(ops):
    from aphrodite_engine_amd import torch_cpp
    torch_cpp.load()
    args, ref = real_case("c", 200, torch.float16)
    close(getattr(torch.ops, torch_cpp.NAMESPACE).gptq_gemm(*args, True, 4), ref, torch.float16)


@pytest.mark.parametrize("m", [129, 200])
def test_wna16_g32_layer(ops, m):
    """compressed-tensors W4A16 (uint4b8: zero point 8 everywhere), group size 32, through the MPLinearKernel seam: 129 rows
    (below WNA16_G32_LARGE_MIN_M: the decode kernel's passes) and 200 rows (the new kernel)."""
    from aphrodite_engine_amd.quantization.kernels.cdna4 import CDNA4LinearKernel
    from aphrodite_engine_amd.quantization.kernels.MPLinearKernel import MPLinearLayerConfig
    from aphrodite_engine_amd.scalar_type import scalar_types
    k, n = CASES["c"]
    rng = np.random.default_rng(11)
    qw = oq.gptq_pack(rng.integers(0, 16, size=(k, n)), 4)       # checkpoint order: the kernel repacks it
    s = rng.uniform(0.002, 0.02, size=(k // GS, n)).astype(np.float32)
    cfg = MPLinearLayerConfig(full_weight_shape=(k, n), partition_weight_shape=(k, n), weight_type=scalar_types.uint4b8,
                              act_type=torch.float16, group_size=GS, zero_points=False, has_g_idx=False)
    kern = CDNA4LinearKernel(cfg, "weight_packed", "weight_scale")
    layer = torch.nn.Module()
    layer.register_parameter("weight_packed", torch.nn.Parameter(dev(qw), requires_grad=False))
    layer.register_parameter("weight_scale", torch.nn.Parameter(dev(s, torch.float16), requires_grad=False))
    kern.process_weights_after_loading(layer)
    a = dev((np.random.default_rng(6).standard_normal((m, k)) * 0.5).astype(np.float32), torch.float16)
    ref = oq.gptq_gemm(a.float().cpu().numpy(), oq.gptq_shuffle(qw), oq.pack_cols(np.full((k // GS, n), 7), 4),
                       layer.weight_scale.float().cpu().numpy(), None, True, 4)
    close(kern.apply_weights(layer, a), ref, torch.float16)
