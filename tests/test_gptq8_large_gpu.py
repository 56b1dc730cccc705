"""The prompt-sized 8-bit GPTQ / uint8b128 GEMM (csrc/gptq8_gemm_large.hip) against the fp64 oracle, through every entry
that reaches it: ops.gptq8_gemm_large, ops.gptq_gemm's routing, HIP-graph replay, the C++ registration, the layer.
Plans at the rows used here (65 / 129): a, b, d run one K slice; c two; e eight (the split-K form: fp32 slabs + reduce);
f two slices of 9 groups each, so every slice crosses the 8-group window of staged scales / zeros; g two slices of ONE
group, so the second begins inside it."""
import functools

import numpy as np
import pytest
import torch

from oracle import quant as oq

pytestmark = pytest.mark.gpu
DEV = "cuda"
#        K     N    gs
CASES = {"a": (64, 128, 64),        # one K tile (pipeline prologue and epilogue only), one column tile
         "b": (192, 384, 64),       # odd number of K tiles, three column tiles, a new group every tile
         "c": (1024, 256, 128),     # groups spanning two K tiles; act-order through perm
         "d": (512, 128, 512),      # channel-wise, groups == 1
         "e": (4096, 128, 128),     # split-K at small M
         "f": (1152, 128, 64),      # more groups in a K slice than one LDS window holds
         "g": (1024, 128, 1024)}    # channel-wise and K-sliced
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
def _weights(name, exact, n=None):
    """Sequential-layout 8-bit weights -> (qweight [K/4, N], qzeros [G, N/4] (stored = zero - 1), scales fp32, perm)."""
    k, n_case, gs = CASES[name]
    n = n or n_case
    rng = np.random.default_rng(ord(name) + n + exact)
    q = rng.integers(0, 256, size=(k, n))
    z = rng.integers(0, 256, size=(k // gs, n))
    q[0, 0], q[1, 0], z[0, 0], z[0, 1] = 0, 255, 0, 255          # stored zero 255 means 256
    s = 2.0 ** -rng.integers(6, 10, size=(k // gs, n)) if exact else rng.uniform(0.002, 0.02, size=(k // gs, n))
    return oq.gptq_pack(q, 8), oq.pack_cols(z, 8), s.astype(np.float32), rng.permutation(k).astype(np.int32)


def exact_case(name, m, dtype):
    """Inputs on which every product and every partial sum is exact in fp32 in any order (see the assert) -> device
    (a, qweight, qzeros, scales) and the fp64 oracle result rounded once to dtype."""
    qw, qz, s, _ = _weights(name, True)
    k, amax = qw.shape[0] * 4, 1 if name == "e" else 2
    assert k * amax * 256 * (2.0 ** -6 / 2.0 ** -9) <= 2 ** 23
    a = np.random.default_rng(m).integers(-amax, amax + 1, size=(m, k)).astype(np.float32)
    ref = torch.from_numpy(oq.gptq_gemm(a, qw, qz, s, None, True, 8)).to(dtype)
    return (dev(a, dtype), dev(qw), dev(qz), dev(s, dtype)), ref


def real_case(name, m, dtype, n=None):
    """-> device (a, qweight, qzeros, scales, perm), fp64 oracle result on the rounded a / scales (act-order through perm)."""
    qw, qz, s, perm = _weights(name, False, n)
    a = dev((np.random.default_rng(m).standard_normal((m, qw.shape[0] * 4)) * 0.5).astype(np.float32), dtype)
    s_t = dev(s, dtype)
    ref = oq.gptq_gemm(a.float().cpu().numpy(), qw, qz, s_t.float().cpu().numpy(), perm, True, 8)
    return (a, dev(qw), dev(qz), s_t, dev(perm)), ref


def close(got, ref, dtype):
    got = got.float().cpu().numpy()
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=TOL[dtype], atol=TOL[dtype] * np.abs(ref).max())


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("m", [65, 129])
@pytest.mark.parametrize("name", list(CASES))
def test_gptq8_large_exact(ops, name, m, dtype):
    """Bit equality: an off-by-one zero point or a misplaced byte cannot hide under a tolerance here."""
    from aphrodite_engine_amd import _lib
    k, n, gs = CASES[name]
    assert ops.gptq8_large_ok(m, n, k, k // gs, dtype)
    if name == "e":      # f16: the workspace is the fp32 slabs alone -> the split form is what runs
        assert _lib.lib().aphro_gptq8_gemm_large_workspace_bytes(m, n, k, k // gs, _lib.F16) == 8 * m * n * 4
    args, ref = exact_case(name, m, dtype)
    assert torch.equal(ops.gptq8_gemm_large(*args).cpu(), ref)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
@pytest.mark.parametrize("m", [129, 256])
@pytest.mark.parametrize("name", ["b", "c"])
def test_gptq8_large_vs_oracle(ops, name, m, dtype):
    (a, qw, qz, s, perm), ref = real_case(name, m, dtype)
    close(ops.gptq8_gemm_large(a[:, perm.long()], qw, qz, s), ref, dtype)


def test_gptq8_large_routing(ops):
    (a, qw, qz, s, perm), ref = real_case("c", 65, torch.float16)
    out = ops.gptq_gemm(a, qw, qz, s, perm, True, 8)
    assert torch.equal(out, ops.gptq8_gemm_large(a[:, perm.long()], qw, qz, s))
    close(out, ref, torch.float16)
    args96, ref96 = real_case("c", 65, torch.float16, n=96)       # no 128-column tiling: gptq_dequant + library GEMM
    assert not ops.gptq8_large_ok(65, 96, 1024, 8, torch.float16)
    close(ops.gptq_gemm(*args96, True, 8), ref96, torch.float16)


def test_gptq8_large_graph_replay(ops):
    """The split-K form (case e) captured once: every replay equals the eager call on the same activations."""
    args, _ = exact_case("e", 65, torch.float16)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.gptq8_gemm_large(*args)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.gptq8_gemm_large(*args)
    for seed in range(3):
        args[0].copy_(torch.randn(args[0].shape, generator=torch.Generator().manual_seed(seed)).to(DEV))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, ops.gptq8_gemm_large(*args))


def test_gptq8_large_cpp_op(ops):
    from aphrodite_engine_amd import torch_cpp
    torch_cpp.load()
    args, ref = real_case("c", 300, torch.float16)
    close(getattr(torch.ops, torch_cpp.NAMESPACE).gptq_gemm(*args, True, 8), ref, torch.float16)


def test_gptq8_large_layer(ops):
    """compressed-tensors W8A16, channel-wise (uint8b128: zero point 128 everywhere), 129 rows through the MPLinearKernel seam."""
    from aphrodite_engine_amd.quantization.kernels.cdna4 import CDNA4LinearKernel
    from aphrodite_engine_amd.quantization.kernels.MPLinearKernel import MPLinearLayerConfig
    from aphrodite_engine_amd.scalar_type import scalar_types
    k, n, _ = CASES["d"]
    qw, _, s, _ = _weights("d", False)
    cfg = MPLinearLayerConfig(full_weight_shape=(k, n), partition_weight_shape=(k, n), weight_type=scalar_types.uint8b128,
                              act_type=torch.float16, group_size=-1, zero_points=False, has_g_idx=False)
    kern = CDNA4LinearKernel(cfg, "weight_packed", "weight_scale")
    layer = torch.nn.Module()
    layer.register_parameter("weight_packed", torch.nn.Parameter(dev(qw), requires_grad=False))
    layer.register_parameter("weight_scale", torch.nn.Parameter(dev(s, torch.float16), requires_grad=False))
    kern.process_weights_after_loading(layer)
    a = dev((np.random.default_rng(6).standard_normal((129, k)) * 0.5).astype(np.float32), torch.float16)
    ref = oq.gptq_gemm(a.float().cpu().numpy(), qw, oq.pack_cols(np.full((1, n), 127), 8),
                       layer.weight_scale.float().cpu().numpy(), None, True, 8)
    close(kern.apply_weights(layer, a), ref, torch.float16)
